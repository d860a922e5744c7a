"""The network's output heads on the device (include/tetris_hip.h: tetris_q_head_dev, tetris_q_head_grad_dev,
tetris_policy_head_dev, tetris_policy_head_grad_dev) against the model of tests/head_support.py, written from the header's
definition: 1. the float64 form of the model against torch autograd of the reference's own lines; 2. bit equality wherever no
library call lies between input and output; 3. everything behind tanhf / expf within derived tolerances of the float64 model, with
planted ties; 4. extreme ranges; 5. the argument rules; 6. on the GPU the TorchEnv wrappers inside a small training step.  Every
test but the first and the last group runs on the CPU harness (`-m "not gpu"`) and on the MI355X (`-m gpu`); on the harness the
"device" buffers are numpy arrays."""
import importlib
import itertools

import numpy as np
import pytest

import __graft_entry__ as ge
from tests import engines
from tests.buffers import GUARD, sync
from tests.head_support import (ALL, F16, F32, F64, SOME, U24, PolicyCall, QCall, half_ulp, policy_backward, policy_forward, policy_inputs,
                                policy_tolerances, q_backward, q_forward, q_inputs, q_tolerances, q_value, ref_action_softmax,
                                ref_policy_value, ref_qva, stored, untouched)

# one sample, the kernel's block of 16 samples and one less and more, a partial wave, 64 and one more, many blocks with a partial last
SIZES = (1, 15, 16, 17, 33, 64, 65, 257)
MODE_SETS = (("mean", True), ("max", True), ("max", False), ("none", True))
K_KV = ((7, 7), (7, 1), (7, 0), (1, 1), (1, 0))
TYPES = (F32, F16)


def _q_cases():
    """every size with every mode and both element types; (K, Kv), the mask and rho rotate with indices of their own, so that none
    of them is tied to the size, the mode or the type"""
    cases = []
    for n, ((mi, M), (ti, dt), (oi, (mode, sep))) in enumerate(itertools.product(enumerate(SIZES), enumerate(TYPES), enumerate(MODE_SETS))):
        K, Kv = K_KV[(n + mi) % 5]
        cases.append((M, mode, sep, K, Kv, (ALL, SOME)[(mi + ti + oi) % 2] if K == 7 else 1, dt, (1.0, 0.5, 0.3)[(n + ti) % 3]))
    for (oi, (mode, sep)), (ki, mask), (ti, dt) in itertools.product(enumerate(MODE_SETS), enumerate((ALL, SOME)), enumerate(TYPES)):
        cases.append((257, mode, sep, 7, (7, 1, 0)[(oi + ki + ti) % 3], mask, dt, (1.0, 0.5)[(oi + ki + ti) % 2]))          # every branch at M = 257
    return list(dict.fromkeys(cases))


Q_CASES = _q_cases()
P_CASES = [(M, K, W, dt) for M, dt in itertools.product(SIZES, TYPES) for K, W in ((7, 8), (7, 1), (1, 2), (1, 1))]


def q_id(c):
    M, mode, sep, K, Kv, mask, dt, rho = c
    return f"M{M}-{mode}{'' if mode != 'max' else '_sep' if sep else '_joint'}-K{K}-Kv{Kv}-used{mask:x}-{np.dtype(dt).name}-rho{rho}"


def p_id(c):
    return f"M{c[0]}-K{c[1]}-W{c[2]}-{np.dtype(c[3]).name}"


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


def run_q(kind, b, inp, mode, sep, mask, rho, **kw):
    call = QCall(kind, b, inp, mode=mode, rho=rho, separate=sep, mask=mask, **kw)
    b.q_head_dev(call.h)
    b.q_head_grad_dev(call.h)
    sync(kind, b)
    return call, call.get()


def run_policy(kind, b, inp, **kw):
    call = PolicyCall(kind, b, inp, **kw)
    b.policy_head_dev(call.h)
    sync(kind, b)
    return call


# ---------------------------------------------------------------- 1. the float64 model against autograd of the reference's lines
# Tolerance.  Every entry of a gradient is a sum of at most 280 terms gd_jk (times factors of magnitude <= 1); the model and autograd
# add them in different orders, each with at most 280 roundings of 2^-53 relative to partial sums of at most sum |G|.  The terms
# themselves agree to a few roundings of the centre c (about 50 roundings of numbers <= 4): 2^-53 * 200 |G|.  Together
# 2 * 280 * 2^-53 sum |G| + 280 * 200 * 2^-53 max |G| <= 280 * 2^-52 (sum |G| + 100 max |G|), taken per sample.
def tol64(G):
    G = np.abs(np.asarray(G, F64)).reshape(G.shape[0], -1)
    return 280 * 2.0 ** -52 * (G.sum(axis=1) + 100 * G.max(axis=1))


@pytest.mark.parametrize("K,Kv", K_KV)
@pytest.mark.parametrize("mask", [ALL, SOME], ids=["all", "some"])
@pytest.mark.parametrize("mode,sep", MODE_SETS, ids=["mean", "max_sep", "max_joint", "none"])
@pytest.mark.parametrize("rho", [1.0, 0.5])
def test_the_float64_model_against_torch_autograd_q(rho, mode, sep, mask, K, Kv):
    """CPU only.  Q, V, A and the gradients of sum G Q with respect to a_raw and v of the float64 model against torch autograd
    (float64) of qva_from_raw_streams transcribed with amax / amin / mean / tanh, on inputs with every planted tie (rho = 1, 0.5
    are exact, so both sides see the same ties)."""
    import torch
    mask = mask if K == 7 else 1
    M = 70
    inp = q_inputs(np.random.default_rng(100 + K + Kv), M, K, Kv, F64)
    m = q_forward(F64, inp["a"], inp["v"], rho, mode, sep, mask, F64)
    m.update(q_backward(F64, inp["a"], inp["G"], rho, mode, sep, mask, Kv))
    a = torch.tensor(inp["a"].reshape(M, 4, 10, K), requires_grad=True)
    v = torch.tensor(inp["v"], requires_grad=True) if Kv else None
    Q, V, A = ref_qva(v.reshape(M, 1, 1, Kv) if Kv else 0.0, a, rho, mode, sep, mask)
    grads = torch.autograd.grad((Q * torch.tensor(inp["G"].reshape(M, 4, 10, K))).sum(), [a] + ([v] if Kv else []))
    tol = tol64(inp["G"])
    for name, got, want in (("Q", m["Q"], Q), ("A", m["A"], A), ("grad_a", m["grad_a"], grads[0])):
        err = np.abs(got - want.detach().numpy().reshape(M, 40, K)).reshape(M, -1).max(axis=1)
        assert (err <= tol).all(), f"{name}: {err.max():.3g} (allowed {tol.min():.3g})"
    assert (np.abs(m["V"] - V.detach().numpy().reshape(M)) <= tol).all()
    if Kv:
        assert (np.abs(m["grad_v"] - grads[1].numpy()).max(axis=1) <= tol).all()
    if mode == "max":
        assert (m["n_max"] > 1).any() and (m["n_lo"] > 1).any(), "the inputs hold no tie"


@pytest.mark.parametrize("K,W", [(7, 8), (7, 1), (1, 2), (1, 1)])
def test_the_float64_model_against_torch_autograd_policy(K, W):
    """CPU only.  pi, v, grad_x, grad_w against autograd of action_softmax and the piece-value head (mask {0, 2, 5}: it cancels)."""
    import torch
    M = 40
    inp = policy_inputs(np.random.default_rng(7 * K + W), M, K, W, F64)
    f = policy_forward(F64, inp["x"], inp["w"])
    bw = policy_backward(F64, f["pi"], f["v"], inp["g"], inp["gv"], W)
    x, w = torch.tensor(inp["x"].reshape(M, 4, 10, K), requires_grad=True), torch.tensor(inp["w"], requires_grad=True)
    pi, v = ref_action_softmax(x), ref_policy_value(w, SOME if K == 7 else 1, K)
    gx, gw = torch.autograd.grad((pi * torch.tensor(inp["g"].reshape(M, 4, 10, K))).sum() + (v * torch.tensor(inp["gv"])).sum(), [x, w])
    tol = tol64(inp["g"])[:, None]
    assert (np.abs(f["pi"] - pi.detach().numpy().reshape(M, 40, K)).reshape(M, -1) <= tol).all()
    assert (np.abs(bw["grad_x"] - gx.numpy().reshape(M, 40, K)).reshape(M, -1) <= tol).all()
    # v = tanh(w_0 + (w_k - c)), |w| <= 2, u = 2^-53: c takes K additions and a division, the argument two more roundings, all of
    # magnitudes <= 4: (K + 3) 4 u, handed on by |tanh'| <= 1; tanh itself within 2 units in the last place of a number below 1 on
    # either side; and both sides round: tol_v = 2 ((K + 3) 4 + 2) u.  grad_w, |gv| <= 1: gt = gv (1 - v v) moves by 2 tol_v and three
    # roundings; T sums K of them with K - 1 roundings of magnitudes <= K, and gt - T / K adds two: (K + 1) (2 tol_v + 3 u) + 2 (K + 1) K u.
    u53 = 2.0 ** -53
    tol_v = 2 * ((K + 3) * 4 + 2) * u53
    tol_w = (K + 1) * (2 * tol_v + 3 * u53) + 2 * (K + 1) * K * u53
    assert (np.abs(f["v"] - v.detach().numpy()) <= tol_v).all() and (np.abs(bw["grad_w"] - gw.numpy()) <= tol_w).all()


# ---------------------------------------------------------------- 2. bit equality
@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("case", P_CASES, ids=p_id)
def test_policy_backward_equals_the_model_bit_for_bit(kind, case, batch_of):
    """grad_x and grad_w from stored pi, v, grad_pi, grad_v carry the float32 model's bits (no library call); every element of both
    is written, nothing behind them.  pi holds exact zeros (underflow): their gradient is exactly zero."""
    M, K, W, dt = case
    b = batch_of(kind)
    inp = policy_inputs(np.random.default_rng(31 * M + K + W), M, K, W, dt)
    f = policy_forward(F64, inp["x"], inp["w"])
    call = PolicyCall(kind, b, inp)
    pi, v = f["pi"].astype(dt), f["v"].astype(dt)
    call.outs["pi"].put(pi)
    call.outs["v"].put(v)
    b.policy_head_grad_dev(call.h)
    sync(kind, b)
    got = call.get("grad_x", "grad_w")
    want = policy_backward(F32, pi, v, inp["g"], inp["gv"], W)
    assert written(got["grad_x"]) and written(got["grad_w"])
    assert same_bits(got["grad_x"], want["grad_x"].astype(dt)) and same_bits(got["grad_w"], want["grad_w"].astype(dt))
    if M >= 3 and K == 7:
        assert (pi == 0).any() and (got["grad_x"][pi == 0] == 0).all()


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("case", Q_CASES, ids=q_id)
def test_q_exact_outputs(kind, case, batch_of):
    """What no library call separates from the call's inputs or from its own outputs, bit for bit:
    V is the model's q_to_v of the stored Q;  grad_v is the model's sums of grad_Q;  with float32 arrays gd = G (1 - A A) from the
    forward call's own A gives the elements of grad_a that take no share — all under NONE, the unused pieces under MEAN (no mean
    share beyond their own gd), the untied elements under MAX — as rho gd exactly (the backward recomputes the forward's A), and
    exact zeros where A = +-1.  Every element of every output is written, nothing behind them."""
    M, mode, sep, K, Kv, mask, dt, rho = case
    b = batch_of(kind)
    inp = q_inputs(np.random.default_rng(17 * M + K + Kv), M, K, Kv, dt, ties=rho != 0.3)
    call, got = run_q(kind, b, inp, mode, sep, mask, rho)
    assert all(written(x) for x in got.values())
    assert same_bits(got["V"], q_value(F32, got["Q"], mask))
    m = q_backward(F32, inp["a"], inp["G"], rho, mode, sep, mask, Kv)
    if Kv:
        assert same_bits(got["grad_v"], m["grad_v"].astype(dt))
    if dt is F32:
        A, G = got["A"], inp["G"]
        gd = G * (F32(1) - A * A)
        if mode == "max":
            plain = ~m["eq_max"] & ~m["eq_lo"] if sep else ~m["eq_max"]
        elif mode == "mean":
            plain = np.broadcast_to(~m["used"][None, None, :], A.shape)
        else:
            plain = np.ones(A.shape, bool)
        assert same_bits(got["grad_a"][plain], (F32(rho) * gd)[plain])
        assert (got["grad_a"][plain & (np.abs(A) == 1)] == 0).all()
        if M == 257 and rho != 0.3 and (mode == "none" or (mode == "mean" and mask == SOME)):
            assert (plain & (A == -1)).any() and (plain & (A == 1)).any(), "no saturated element among those checked"


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("dt", TYPES, ids=["float32", "float16"])
def test_grad_a_does_not_depend_on_v_and_without_v_no_grad_v_is_written(kind, dt, batch_of):
    b = batch_of(kind)
    inp = q_inputs(np.random.default_rng(5), 65, 7, 7, dt)
    _, with_v = run_q(kind, b, inp, "max", True, SOME, 0.5)
    _, without = run_q(kind, b, dict(inp, v=None), "max", True, SOME, 0.5)
    assert same_bits(with_v["grad_a"], without["grad_a"]) and same_bits(with_v["A"], without["A"]) and "grad_v" not in without
    assert same_bits(without["Q"], without["A"]), "v == NULL stands for 0"
    skip_A, _ = run_q(kind, b, inp, "max", True, SOME, 0.5, want_A=False)
    assert same_bits(skip_A.get("Q")["Q"], with_v["Q"])


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
def test_the_value_arrays_have_a_flag_of_their_own(kind, batch_of):
    """binary16 big arrays with float32 value arrays, and the other way round, against the float64 model"""
    b = batch_of(kind)
    for big, small in ((F16, F32), (F32, F16)):
        inp = q_inputs(np.random.default_rng(6), 33, 7, 7, big)
        inp["v"] = inp["v"].astype(small)
        _, got = run_q(kind, b, inp, "mean", True, ALL, 1.0)
        m = q_forward(F64, inp["a"], inp["v"], 1.0, "mean", True, ALL, big)
        assert got["grad_v"].dtype == small and same_bits(got["grad_v"], q_backward(F32, inp["a"], inp["G"], 1.0, "mean", True, ALL, 7)["grad_v"].astype(small))
        assert (np.abs(got["Q"].astype(F64) - m["Q"]) <= q_tolerances(m, inp["v"])["Q"][:, None, None] + half_ulp(m["Q"], big)).all()
        pin = policy_inputs(np.random.default_rng(7), 33, 7, 8, big)
        pin["w"], pin["gv"] = pin["w"].astype(small), pin["gv"].astype(small)
        call = run_policy(kind, b, pin)
        f = policy_forward(F64, pin["x"], pin["w"])
        got = call.get("pi", "v")
        assert got["v"].dtype == small and (np.abs(got["v"].astype(F64) - f["v"]) <= policy_tolerances(f, pin["w"])["v"][:, None] + half_ulp(f["v"], small)).all()


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
def test_a_second_call_gives_the_same_bytes(kind, batch_of):
    b = batch_of(kind)
    for dt in TYPES:
        inp = q_inputs(np.random.default_rng(8), 257, 7, 1, dt)
        call, first = run_q(kind, b, inp, "max", False, SOME, 0.5)
        b.q_head_dev(call.h)
        b.q_head_grad_dev(call.h)
        pin = policy_inputs(np.random.default_rng(9), 257, 7, 8, dt)
        pc = run_policy(kind, b, pin)
        b.policy_head_grad_dev(pc.h)
        sync(kind, b)
        pfirst = pc.get()
        b.policy_head_dev(pc.h)
        b.policy_head_grad_dev(pc.h)
        sync(kind, b)
        again, pagain = call.get(), pc.get()
        assert all(first[n].tobytes() == again[n].tobytes() for n in first) and all(pfirst[n].tobytes() == pagain[n].tobytes() for n in pfirst)


# ---------------------------------------------------------------- 3. and 4. behind tanhf / expf: the float64 model, derived tolerances
@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("case", Q_CASES, ids=q_id)
def test_q_head_lies_within_the_tolerance_of_the_float64_model(kind, case, batch_of):
    """Q, A, V, grad_a and grad_v against the float64 form of the model, head_support.q_tolerances apart at most (binary16 outputs:
    half a unit in their last place more).  The float32 and float64 forms report identical tie sets, so a tie that one of them
    misses cannot hide as tolerance.  At M = 257 (rho = 1, 0.5) every planted tie and range occurred: two equal maxima, an
    all-equal plane, the minimum twice, the minimum inside a used and inside an unused piece, |d| > 10 with A = -1 exactly (and
    A = +1 where the mode allows d > 10)."""
    M, mode, sep, K, Kv, mask, dt, rho = case
    b = batch_of(kind)
    inp = q_inputs(np.random.default_rng(17 * M + K + Kv), M, K, Kv, dt, ties=rho != 0.3)
    _, got = run_q(kind, b, inp, mode, sep, mask, rho)
    m32 = q_backward(F32, inp["a"], inp["G"], rho, mode, sep, mask, Kv)
    m = q_forward(F64, inp["a"], inp["v"], rho, mode, sep, mask, dt)
    m.update(q_backward(F64, inp["a"], inp["G"], rho, mode, sep, mask, Kv))
    for name in ("eq_max", "eq_lo", "n_max", "n_lo"):
        assert np.array_equal(m32[name], m[name]), f"the two forms of the model disagree on {name}"
    tol = q_tolerances(m, inp["v"], inp["G"])
    worst = {}
    for name in ("A", "Q", "grad_a"):
        err = np.abs(got[name].astype(F64) - m[name])
        allowed = tol[name][:, None, None] + half_ulp(m[name], dt)
        worst[name] = float((err / allowed).max())
        assert (err <= allowed).all(), f"{name}: {err.max():.3g}"
    # V: the error of the stored Q's maxima, a sum of at most 7 of them and a division
    errV = np.abs(got["V"].astype(F64) - q_value(F64, stored(m["Q"], dt), mask))
    assert (errV <= tol["Q"] + half_ulp(np.abs(m["Q"]).reshape(M, -1).max(axis=1), dt) + 8 * U24 * 2).all()
    if Kv:
        assert (np.abs(got["grad_v"].astype(F64) - m["grad_v"]) <= tol["grad_v"][:, None] + half_ulp(m["grad_v"], dt)).all()
    print(f"largest share of the tolerance: {worst}")
    if M == 257 and rho != 0.3:
        kinds = set(inp["kind"].tolist())
        assert kinds == set(range(7))
        A = got["A"].astype(F64)
        assert (A == -1).any()
        if mode in ("mean", "none"):
            assert (A == 1).any()
        if mode == "max":
            used = m["used"]
            assert (m["n_max"][:, used] == 2).any() and (m["n_max"][:, used] == 40).any() and (m["n_lo"] == 2).any()
            if mask == SOME:
                lo_in_unused = (m["eq_lo"] & ~used[None, None, :]).any(axis=(1, 2))
                lo_in_used = (m["eq_lo"] & used[None, None, :]).any(axis=(1, 2))
                assert (lo_in_unused & lo_in_used).any() and (lo_in_used & ~lo_in_unused & (m["n_lo"] == 2)).any()


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("case", P_CASES, ids=p_id)
def test_policy_head_lies_within_the_tolerance_of_the_float64_model(kind, case, batch_of):
    """pi and v against the float64 model within head_support.policy_tolerances; pi is finite, sums to 1 within the bound, and
    where the float64 value lies below the element type's smallest number the entry is exactly 0; logits of +-80 in one plane."""
    M, K, W, dt = case
    b = batch_of(kind)
    inp = policy_inputs(np.random.default_rng(31 * M + K + W), M, K, W, dt)
    call = run_policy(kind, b, inp)
    got = call.get("pi", "v")
    assert written(got["pi"]) and written(got["v"])
    f = policy_forward(F64, inp["x"], inp["w"])
    tol = policy_tolerances(f, inp["w"])
    pi = got["pi"].astype(F64)
    assert np.isfinite(pi).all() and (pi >= 0).all()
    assert (np.abs(pi - f["pi"]) <= tol["pi"] + half_ulp(f["pi"], dt)).all()
    assert (np.abs(pi.sum(axis=1) - 1) <= tol["pi_sum"] + 40 * half_ulp(np.ones(1), dt)).all()
    assert (np.abs(got["v"].astype(F64) - f["v"]) <= tol["v"][:, None] + half_ulp(f["v"], dt)).all()
    tiny = f["pi"] < (2.0 ** -150 if dt is F32 else 2.0 ** -26)
    assert (pi[tiny] == 0).all()
    if M == 257 and K == 7:
        assert tiny.any() and (np.abs(inp["x"].astype(F64)).max() == 80)


# ---------------------------------------------------------------- 5. the argument rules
# (what is wrong, the argument that makes it so, the words of its message, the direction it concerns: both where none is named).  Every
# rule is refused with TETRIS_E_ARG, the one code the C ABI has for a bad argument; what tells the rules apart is the message.
Q_RULES = [("M = 0", dict(m=0), "M < 1"), ("M < 0", dict(m=-3), "M < 1"), ("K = 3", dict(n_pieces=3), "n_pieces must be 1 or 7"),
           ("Kv = 2", dict(n_values=2), "n_values must be 1 or n_pieces"), ("an unknown mode", dict(mode=3), "mode must be"),
           ("no used piece", dict(used_pieces=0), "names no piece"), ("a used piece at K", dict(used_pieces=0x80), "at or above n_pieces"),
           ("an unknown flag", dict(flags=4), "unknown flag"), ("a is NULL", dict(a=None), "a is NULL"),
           ("Q is NULL", dict(Q=None), "Q/V are NULL", "fwd"), ("V is NULL", dict(V=None), "Q/V are NULL", "fwd"),
           ("grad_Q is NULL", dict(grad_Q=None), "grad_Q/grad_a are NULL", "bwd"), ("grad_a is NULL", dict(grad_a=None), "grad_Q/grad_a are NULL", "bwd"),
           ("grad_v is NULL", dict(grad_v=None), "grad_v is NULL where v is given", "bwd")]
P_RULES = [("M = 0", dict(m=0), "M < 1"), ("M < 0", dict(m=-1), "M < 1"), ("K = 3", dict(n_pieces=3), "n_pieces must be 1 or 7"),
           ("W = 7", dict(n_values=7), "n_values must be 1 or n_pieces + 1"), ("W = 2", dict(n_values=2), "n_values must be 1 or n_pieces + 1"),
           ("an unknown flag", dict(flags=8), "unknown flag"), ("pi is NULL", dict(pi=None), "pi/v are NULL"), ("v is NULL", dict(v=None), "pi/v are NULL"),
           ("x is NULL", dict(x=None), "x/w are NULL", "fwd"), ("w is NULL", dict(w=None), "x/w are NULL", "fwd"),
           ("grad_pi is NULL", dict(grad_pi=None), "grad_pi/grad_v/grad_x/grad_w are NULL", "bwd"),
           ("grad_v is NULL", dict(grad_v=None), "grad_pi/grad_v/grad_x/grad_w are NULL", "bwd"),
           ("grad_x is NULL", dict(grad_x=None), "grad_pi/grad_v/grad_x/grad_w are NULL", "bwd"),
           ("grad_w is NULL", dict(grad_w=None), "grad_pi/grad_v/grad_x/grad_w are NULL", "bwd")]


def refused(pkg, fn, h):
    with pytest.raises(pkg.TetrisError) as e:
        fn(h)
    return str(e.value)


def nothing_written(call):
    """no byte of any output of the call was touched: all still hold the guard pattern"""
    return all(untouched(buf) for buf in call.outs.values())


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
def test_bad_arguments_are_refused(kind, batch_of):
    """every rule on its own, refused with its own message, and no output byte touched (guard-filled buffers); K = 1 takes no mask
    but 1; a NULL struct; each big array 4 bytes off its alignment"""
    pkg, b = ge.package(), batch_of(kind)
    qin, pin = q_inputs(np.random.default_rng(1), 5, 7, 7, F32), policy_inputs(np.random.default_rng(2), 5, 7, 8, F32)
    for rules, Call, fwd, bwd in ((Q_RULES, QCall, b.q_head_dev, b.q_head_grad_dev), (P_RULES, PolicyCall, b.policy_head_dev, b.policy_head_grad_dev)):
        for rule in rules:
            call = Call(kind, b, qin if Call is QCall else pin, **rule[1])
            for which, fn in (("fwd", fwd), ("bwd", bwd)):
                if len(rule) == 3 or rule[3] == which:
                    assert rule[2] in refused(pkg, fn, call.h), f"{rule[0]} ({which})"
            sync(kind, b)
            assert nothing_written(call), rule[0]
    one = QCall(kind, b, q_inputs(np.random.default_rng(3), 5, 1, 1, F32), used_pieces=3)
    assert "at or above n_pieces" in refused(pkg, b.q_head_dev, one.h) and nothing_written(one)
    for fn in (b.q_head_dev, b.q_head_grad_dev, b.policy_head_dev, b.policy_head_grad_dev):
        assert "the argument struct is NULL" in refused(pkg, fn, None)
    for name, fns in (("a", (b.q_head_dev, b.q_head_grad_dev)), ("G", (b.q_head_grad_dev,)), ("Q", (b.q_head_dev,)), ("A", (b.q_head_dev,)),
                      ("grad_a", (b.q_head_grad_dev,))):
        call = QCall(kind, b, qin, offsets={name: 4})
        for fn in fns:
            assert "16-byte aligned" in refused(pkg, fn, call.h), name
        sync(kind, b)
        assert nothing_written(call), name
    for name, fns in (("x", (b.policy_head_dev,)), ("pi", (b.policy_head_dev, b.policy_head_grad_dev)), ("g", (b.policy_head_grad_dev,)),
                      ("grad_x", (b.policy_head_grad_dev,))):
        call = PolicyCall(kind, b, pin, offsets={name: 4})
        for fn in fns:
            assert "16-byte aligned" in refused(pkg, fn, call.h), name
        sync(kind, b)
        assert nothing_written(call), name


# ---------------------------------------------------------------- 6. TorchEnv: the wrappers inside a small training step (GPU only)
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_torch_heads_inside_a_training_step(dtype):
    """A linear "trunk" gives (_V, _A) and (x, w) for M = 65 samples; te.dqn_loss(te.q_head(...)[0], ...) and
    te.ppo_loss(*te.policy_head(...), ...) are run backward, and the gradient that reaches the trunk's output, and through the
    linear layer its weights, is compared with the same step composed from torch ops in float32 (the reference's lines of
    head_support) and the same loss heads.  V and A are non-differentiable.
    Tolerance of an element of the trunk output's gradient, relative to the largest one: the heads' bounds of section 3 for these
    magnitudes — |a| <= 3, so E_A = (51 * 3 + 5) u = 9.4e-6 and E_g = 2 E_A + 3 u = 1.9e-5 relative to |G|, the 280-term shares the
    same relative to sum |G| — times SAFETY = 4: 1e-4 covers both compositions' float32 roundings.  float16 (streams and gradients
    in binary16, grad_scale = 128): the two paths round the gradient to binary16 at the same place but from different float32
    values, one unit of binary16 (2^-10) more.  A weight's gradient sums M elements times features in [0, 1]: the element bound
    times the largest column sum of the features."""
    import torch
    pkg = ge.package()
    M, K, F = 65, 7, 12
    dt = getattr(torch, dtype)
    scale = 128.0 if dtype == "float16" else 1.0
    rel = 1e-4 + (2.0 ** -10 if dtype == "float16" else 0.0)
    b = pkg.TetrisBatch(M, 1, 8, 10, device=0)
    try:
        te = importlib.import_module("drl-tetris_amd.torch_interop").TorchEnv(b)
        g = torch.Generator(device="cpu").manual_seed(3)
        feat = torch.rand(M, F, generator=g).cuda()
        action = torch.stack([torch.randint(0, 4, (M,), generator=g), torch.randint(0, 10, (M,), generator=g),
                              torch.randint(0, 7, (M,), generator=g)], 1).to(torch.uint8).cuda()
        target = torch.rand(M, generator=g).cuda()
        old, adv = (0.02 + 0.05 * torch.rand(M, generator=g)).cuda(), torch.randn(M, generator=g).cuda()
        params = dict(clipping_parameter=0.15, value_loss=1.0, policy_loss=1.0, entropy_loss=0.01, ppo_epsilon=0.05, entropy_floor_loss=0.0,
                      rescaled_entropy=0.0)
        for head in ("q", "policy"):
            width = 40 * K + (K if head == "q" else K + 1)
            W0 = (0.15 * torch.randn(F, width, generator=g)).cuda()
            grads = {}
            for how in ("device", "torch"):
                W = W0.clone().requires_grad_(True)
                raw = (feat @ W).to(dt)
                raw.retain_grad()
                big, small = raw[:, :40 * K].reshape(M, 4, 10, K).contiguous(), raw[:, 40 * K:].contiguous()
                if head == "q":
                    if how == "device":
                        Q, V, A = te.q_head(big, small, mode="max", advantage_range=0.5, separate_piece_values=False, pieces=SOME, A=True)
                        assert not V.requires_grad and not A.requires_grad and Q.requires_grad
                    else:
                        Q = ref_qva(small.float().reshape(M, 1, 1, K), big.float(), 0.5, "max", False, SOME)[0].to(dt)
                    loss = te.dqn_loss(Q.contiguous(), action, target, grad_scale=scale)[0]
                else:
                    if how == "device":
                        pi, v = te.policy_head(big, small)
                    else:
                        pi, v = ref_action_softmax(big.float()).to(dt), ref_policy_value(small.float(), SOME, K).to(dt)
                    loss = te.ppo_loss(pi.contiguous(), v.contiguous(), action, old, adv, target, grad_scale=scale, **params)[0]
                loss.backward()
                grads[how] = (raw.grad.double().cpu().numpy() / scale, W.grad.double().cpu().numpy() / scale)
            (dev_raw, dev_w), (ref_raw, ref_w) = grads["device"], grads["torch"]
            bound = rel * np.abs(ref_raw).max()
            bound_w = bound * float(feat.sum(dim=0).max())
            err, err_w = np.abs(dev_raw - ref_raw).max(), np.abs(dev_w - ref_w).max()
            print(f"{head} {dtype}: trunk output {err:.3g} (allowed {bound:.3g}), weights {err_w:.3g} (allowed {bound_w:.3g})")
            assert np.abs(ref_raw).max() > 0 and err <= bound and err_w <= bound_w, head
    finally:
        b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_torch_q_head_without_a_value_stream(dtype):
    """te.q_head(a, None, ...) — prio_qnet's full_network=False: _V is the constant 0 — through the wrapper: Q, V and the gradient
    with respect to a against the torch composition in float32 with _V = 0.0, M = 65, MEAN with the mask {0, 2, 5}.  Tolerance as in
    the training-step test: 1e-4 of the largest value (float16: one unit of binary16, 2^-10, more)."""
    import torch
    pkg = ge.package()
    M, K = 65, 7
    dt = getattr(torch, dtype)
    rel = 1e-4 + (2.0 ** -10 if dtype == "float16" else 0.0)
    b = pkg.TetrisBatch(M, 1, 8, 10, device=0)
    try:
        te = importlib.import_module("drl-tetris_amd.torch_interop").TorchEnv(b)
        g = torch.Generator(device="cpu").manual_seed(5)
        a0 = (4 * torch.rand(M, 4, 10, K, generator=g) - 2).to(dt).cuda()
        G = (2 * torch.rand(M, 4, 10, K, generator=g) - 1).to(dt).cuda()
        a = a0.clone().requires_grad_(True)
        Q, V = te.q_head(a, None, mode="mean", advantage_range=0.5, pieces=SOME)
        assert Q.requires_grad and not V.requires_grad
        (ga,) = torch.autograd.grad(Q, (a,), G)
        r = a0.float().requires_grad_(True)
        Qr, Vr, _ = ref_qva(0.0, r, 0.5, "mean", True, SOME)
        (gr,) = torch.autograd.grad(Qr, (r,), G.float())
        for name, got, want in (("Q", Q, Qr), ("V", V, Vr.reshape(M)), ("grad_a", ga, gr)):
            err, top = float((got.detach().float() - want.detach()).abs().max()), float(want.detach().abs().max())
            print(f"{name} {dtype}: largest difference {err:.3g}, allowed {rel * top:.3g}")
            assert top > 0 and err <= rel * top, name
    finally:
        b.close()
