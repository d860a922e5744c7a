"""Acting on a network's (r, t, piece) evaluation on the device (include/tetris_hip.h: tetris_select_eval_dev,
tetris_step_eval_dev, tetris_step_eval_observe_dev) against a model written in tests/act_support.py from the header's definitions: numpy float32
with explicit sequential loops for the sums, oracle.philox for the words, a stable double argsort for the ranks, the oracle for
the boards.  The model owes nothing to drl-tetris_amd/csrc/tetris_act.h.  Every comparison is exact equality (floats by their
bits) except the entropy.  Every test runs on the CPU harness (`-m "not gpu"`) and on the MI355X (`-m gpu`); on the harness the
"device" buffers are numpy arrays.  (The reference's sventon_utils.py is restated, not imported: it needs tensorflow.)"""
import itertools

import numpy as np
import pytest

import __graft_entry__ as ge
from oracle import oracle as orc
from tests import engines
from tests.act_support import Call, assert_outputs, m_ranks, midgame, model, pieces_of, random_maps
from tests.buffers import Buf, bits

F32 = np.float32
MODES = ("argmax", "pi", "rank", "epsilon")


def pareto(theta=1.0):
    return (np.arange(1, 41, dtype=np.float64) ** -theta).astype(F32)


# ---------------------------------------------------------------- 1. choice
# N: a single game, a partial wave, a whole block of 64, a block and one game, several blocks with a partial last one;
# K, the element type: the four forms of the gather; players and heights go round with them
SHAPES = [(n, K, dt, 1 + k % 3, (20, 22)[k % 2]) for k, (n, K, dt) in enumerate(itertools.product((1, 63, 64, 65, 200), (7, 1), (np.float32, np.float16)))]


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("n,K,dtype,P,height", SHAPES, ids=[f"n{n}-K{K}-{np.dtype(dt).name}-P{P}-H{h}" for n, K, dt, P, h in SHAPES])
def test_choice_equals_the_model(kind, n, K, dtype, P, height):
    rng = np.random.default_rng(1000 + n + K)
    b, o = midgame(kind, n, P, height)
    ids = np.arange(n)
    player = rng.integers(0, P, n).astype(np.uint8) if P > 1 else None
    piece_idx = pieces_of(o, np.zeros(n, np.int64) if player is None else player)
    if n >= 63:
        assert len(np.unique(piece_idx)) == 7, "the boards of this test do not hold all seven pieces"
    V = (7, 8, 1)[(n + K) % 3]
    state_eval = rng.standard_normal((n, V)).astype(dtype)
    ties = branches = 0
    for draw, (maps, mode) in enumerate(itertools.product(("normal", "levels", "pi"), MODES)):
        ae = random_maps(rng, n, K, dtype, maps)
        kw = dict(seed=77, draw=draw, epsilon=0.3, table=pareto(1.0) if mode == "rank" else None)
        call = Call(kind, b, ae, mode, player=player, state_eval=state_eval, **kw)
        b.select_eval_dev(call.e)
        want = model(ae, piece_idx, ids, mode, state_eval=state_eval, **kw)
        got = call.get()
        assert_outputs(got, want, f"{maps} maps, {mode}")
        if maps == "levels" and mode == "argmax":
            x = ae.reshape(n, 40, K)[np.arange(n), :, want["piece"]]
            ties += int(((x == x.max(axis=1, keepdims=True)).sum(axis=1) > 1).sum())
        if mode == "epsilon":
            branches |= 1 if want["random"].any() else 0
            branches |= 2 if (~want["random"]).any() else 0
    assert ties > 0, "no map of this test has more than one best candidate"
    if n >= 63:
        assert branches == 3, "epsilon 0.3 did not take both branches"
    engines.assert_same_state(b, o, where="the selection must not write the state")


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("dtype", [np.float32, np.float16], ids=["float32", "float16"])
def test_every_candidate_is_reachable_and_the_piece_gather_is_right(kind, dtype):
    """Game i has its only positive entry at candidate i mod 40 of ITS piece's slice and one at another candidate in every other
    slice: all four modes land on (c / 10, c mod 10).  Then random maps whose maximum sits only in the other pieces' slices."""
    n, P = 80, 2
    rng = np.random.default_rng(5)
    b, o = midgame(kind, n, P)
    player = rng.integers(0, P, n).astype(np.uint8)
    piece_idx = pieces_of(o, player)
    assert len(np.unique(piece_idx)) == 7
    ae = np.zeros((n, 40, 7), dtype)
    cand = np.arange(n) % 40
    for k in range(7):
        ae[np.arange(n), (cand + 1 + k) % 40, k] = 2.0
    ae[np.arange(n), :, piece_idx] = 0.0
    ae[np.arange(n), cand, piece_idx] = 1.0
    ae = ae.reshape(n, 4, 10, 7)
    first = np.zeros(40, F32)
    first[0] = 1.0
    for mode in MODES:
        call = Call(kind, b, ae, mode, player=player, seed=3, draw=9, epsilon=0.0, table=first if mode == "rank" else None)
        b.select_eval_dev(call.e)
        got = call.get()
        assert np.array_equal(got["rot"], cand // 10) and np.array_equal(got["trans"], cand % 10), mode
        assert np.array_equal(got["piece"], piece_idx) and np.array_equal(got["eval"], np.ones(n, F32)), mode
    ae = rng.random((n, 4, 10, 7)).astype(dtype)
    other = np.ones((n, 7), bool)
    other[np.arange(n), piece_idx] = False
    ae = (ae + 10.0 * other[:, None, None, :]).astype(dtype)
    for mode in ("argmax", "pi"):
        call = Call(kind, b, ae, mode, player=player, seed=3, draw=10)
        b.select_eval_dev(call.e)
        got = call.get()
        assert_outputs(got, model(ae, piece_idx, np.arange(n), mode, seed=3, draw=10), f"maximum elsewhere, {mode}")
        assert (got["eval"] < 1.5).all()


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("dtype", [np.float32, np.float16], ids=["float32", "float16"])
def test_fall_backs_to_argmax(kind, dtype):
    """A total that is not a positive finite number gives ARGMAX's choice: PI maps that are all zero, all negative, hold a +inf;
    a NaN entry has the weight 0; all NaN chooses 0.  RANK with a table that is all zero, holds a NaN, holds a +inf."""
    n = 65
    rng = np.random.default_rng(6)
    b, o = midgame(kind, n, 1)
    piece_idx = pieces_of(o, np.zeros(n, np.int64))
    ids = np.arange(n)
    ae = random_maps(rng, n, 7, np.float32, "pi")
    ae[0::6] = 0.0
    ae[1::6, 1, 3, :] = np.nan
    ae[2::6, 2, 4, :] = np.inf
    ae[3::6] = np.nan
    ae[4::6] = -np.abs(ae[4::6]) - 0.5
    ae = ae.astype(dtype)
    want_max = model(ae, piece_idx, ids, "argmax")
    for mode in ("argmax", "pi", "epsilon"):
        call = Call(kind, b, ae, mode, seed=8, draw=2, epsilon=0.5, entropy=False)
        b.select_eval_dev(call.e)
        got = call.get()
        want = model(ae, piece_idx, ids, mode, seed=8, draw=2, epsilon=0.5)
        assert_outputs(got, want, mode)
        if mode == "pi":
            for first in (0, 2, 3, 4):
                assert np.array_equal(got["rot"][first::6], want_max["rot"][first::6]) and np.array_equal(got["trans"][first::6], want_max["trans"][first::6])
            assert not got["rot"][3::6].any() and not got["trans"][3::6].any()
    ae = random_maps(rng, n, 7, dtype, "levels")
    want_max = model(ae, piece_idx, ids, "argmax")
    for bad in (0.0, np.nan, np.inf):
        table = pareto(1.0)
        table[:] = table if bad != 0.0 else 0.0
        table[7] = bad
        call = Call(kind, b, ae, "rank", seed=8, draw=3, table=table)
        b.select_eval_dev(call.e)
        assert_outputs(call.get(), want_max, f"rank table with {bad}")


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
def test_epsilon_zero_one_and_between(kind):
    n = 200
    rng = np.random.default_rng(7)
    b, o = midgame(kind, n, 2, steps=10)
    player = rng.integers(0, 2, n).astype(np.uint8)
    piece_idx = pieces_of(o, player)
    ae = random_maps(rng, n, 7, np.float32, "normal")
    for eps in (0.0, 1.0, 0.3):
        call = Call(kind, b, ae, "epsilon", player=player, seed=11, draw=4, epsilon=eps)
        b.select_eval_dev(call.e)
        want = model(ae, piece_idx, np.arange(n), "epsilon", seed=11, draw=4, epsilon=eps)
        assert_outputs(call.get(), want, f"epsilon {eps}")
        assert want["random"].sum() == {0.0: 0, 1.0: n}.get(eps, want["random"].sum())
        if eps == 0.3:
            assert 0 < want["random"].sum() < n, "epsilon 0.3 did not take both branches"


# ---------------------------------------------------------------- 2. stream
@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
def test_the_sample_stream_is_keyed_by_seed_game_and_draw(kind):
    n, m = 200, 64
    rng = np.random.default_rng(20)
    seeds = orc.episode_seed(np.arange(n), 0)
    big = engines.make(kind, n, 1, seeds=seeds)
    small = engines.make(kind, m, 1, seeds=seeds[:m])
    ae = rng.random((n, 4, 10, 1)).astype(F32)                 # K = 1: the map does not depend on the boards
    zero = np.zeros(n, np.int64)

    def run(b, maps, mode="pi", **kw):
        call = Call(kind, b, maps, mode, **kw)
        b.select_eval_dev(call.e)
        got = call.get()
        return 10 * got["rot"].astype(np.int64) + got["trans"]

    first = run(big, ae, seed=1, draw=5)
    assert np.array_equal(first, model(ae, zero, np.arange(n), "pi", seed=1, draw=5)["c"])
    assert np.array_equal(run(big, ae, seed=1, draw=5), first), "the same (seed, draw) must repeat its choices"
    assert (run(big, ae, seed=1, draw=6) != first).sum() > n // 2, "another draw must change the choices"
    assert (run(big, ae, seed=2, draw=5) != first).sum() > n // 2, "another seed must change the choices"
    high = run(big, ae, seed=1, draw=5 + (1 << 32))
    assert np.array_equal(high, model(ae, zero, np.arange(n), "pi", seed=1, draw=5 + (1 << 32))["c"]) and (high != first).any()
    small.set_game_offset(64)
    assert np.array_equal(run(small, ae[64:128], seed=1, draw=5), first[64:128]), "a batch at offset 64 must equal games 64.. of a larger one"
    big.set_game_offset(7)
    shifted = run(big, ae, seed=1, draw=5)
    assert np.array_equal(shifted, model(ae, zero, np.arange(n) + 7, "pi", seed=1, draw=5)["c"]) and (shifted != first).any()
    eps = run(big, ae, mode="epsilon", seed=1, draw=5, epsilon=1.0)
    assert np.array_equal(eps, model(ae, zero, np.arange(n) + 7, "epsilon", seed=1, draw=5, epsilon=1.0)["c"])


# ---------------------------------------------------------------- 3. distribution
@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("mode", ["pi", "rank"])
def test_distribution_of_the_draw(kind, mode):
    """One fixed map for 16 384 games: the chi-square statistic of the 40 counts against N m[c] / total stays below 72.05, the
    0.999 quantile at 39 degrees of freedom.  The seed is fixed, so the test is deterministic; the exact-equality tests are the
    real check, this one guards the definition itself against a biased u."""
    n = 16384
    b = engines.make(kind, n, 1, seeds=orc.episode_seed(np.arange(n), 0))
    one = ((np.arange(40) * 7) % 11 + 1).astype(F32)                   # weights 1..11, no order along c
    ae = np.ascontiguousarray(np.broadcast_to(one.reshape(1, 4, 10, 1), (n, 4, 10, 1)))
    table = pareto(1.0)
    m = one.astype(np.float64) if mode == "pi" else table[m_ranks(one) - 1].astype(np.float64)
    expected = n * m / m.sum()
    assert expected.min() >= 5
    call = Call(kind, b, ae, mode, seed=2024, draw=1, table=table if mode == "rank" else None)
    b.select_eval_dev(call.e)
    got = call.get()
    counts = np.bincount(10 * got["rot"].astype(np.int64) + got["trans"], minlength=40)
    chi2 = float(((counts - expected) ** 2 / expected).sum())
    print(f"{mode}: chi-square {chi2:.2f} (bound 72.05)")
    assert counts.sum() == n and chi2 < 72.05


# ---------------------------------------------------------------- 4. entropy
@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("dtype", [np.float32, np.float16], ids=["float32", "float16"])
def test_entropy_of_pi(kind, dtype):
    """Against the formula in float64, absolute tolerance 5e-5: 40 terms, each |q log q| <= 0.368 with a relative error of at most
    about 1.7e-7 (an input rounding, a 1-ulp logf, a product rounding), and 40 partial-sum roundings below 3.7 adding 4.8e-6:
    about 1.2e-5 in all; 5e-5 is four times that.  The inputs are normalised probability maps."""
    n = 65
    rng = np.random.default_rng(40)
    b, o = midgame(kind, n, 1, steps=12)
    p = rng.random((n, 7, 40)) ** 3
    ae = np.ascontiguousarray((p / p.sum(axis=2, keepdims=True)).transpose(0, 2, 1)).reshape(n, 4, 10, 7).astype(dtype)
    call = Call(kind, b, ae, "pi", seed=1, draw=0)
    b.select_eval_dev(call.e)
    got = call.get()
    want = model(ae, pieces_of(o, np.zeros(n, np.int64)), np.arange(n), "pi", seed=1, draw=0)
    assert_outputs(got, want, "pi")
    err = np.abs(got["entropy"].astype(np.float64) - want["entropy"])
    print(f"entropy: largest error {err.max():.3g}, values {want['entropy'].min():.3f}..{want['entropy'].max():.3f}")
    assert want["entropy"].min() > 1.0 and err.max() < 5e-5


# ---------------------------------------------------------------- 5. step
@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("P,height,colours", [(1, 20, False), (2, 20, False), (2, 22, False), (3, 20, False), (1, 20, True)])
def test_step_eval_equals_select_plus_step_and_the_oracle(kind, P, height, colours):
    """40 steps with auto-reset, draw = step, the four modes in turn: step_eval_dev against select_eval_dev + step_rt_dev on a
    copy and against the oracle stepped with the model's (r, t); step_eval_observe_dev (one and two players) against
    step_eval_dev followed by the packed observation of the next player."""
    n, steps = 70, 40
    rng = np.random.default_rng(500 + P + height)
    observe = P <= 2
    a, c, d, o = midgame(kind, n, P, height, colours=colours, extra=2)
    ids = np.arange(n)
    episode = np.zeros(n, np.int64)
    ended = 0
    outs = [dict(done=Buf(kind, np.full(n, 7, np.uint8)), lines=Buf(kind, np.full((P, n), 7, np.uint8)), dead=Buf(kind, np.full((P, n), 7, np.uint8)))
            for _ in range(3)]
    obs = dict(visual=Buf(kind, np.zeros((P, n, height, 10), np.uint8)), vector=Buf(kind, np.zeros((P, n, 12), np.uint8)), piece=Buf(kind, np.zeros((P, n), np.uint8)))
    for s in range(steps):
        mode = MODES[s % 4]
        player = rng.integers(0, P, n).astype(np.uint8)
        nxt = rng.integers(0, P, n).astype(np.uint8)
        ae = random_maps(rng, n, 7, np.float32, "normal" if s % 3 else "pi")
        kw = dict(seed=9, draw=s, epsilon=0.5, table=pareto(1.0) if mode == "rank" else None)
        want = model(ae, pieces_of(o, player), ids, mode, **kw)
        calls = [Call(kind, b, ae, mode, player=player, **kw) for b in (a, c, d)]
        oa, oc, od = outs
        a.step_eval_dev(calls[0].e, oa["done"].ptr, oa["lines"].ptr, oa["dead"].ptr, auto_reset=True)
        c.select_eval_dev(calls[1].e)
        c.step_rt_dev(calls[1].out["rot"].ptr, calls[1].out["trans"].ptr, calls[1].pl.ptr, oc["done"].ptr, oc["lines"].ptr, oc["dead"].ptr, auto_reset=True)
        if observe:
            nb = Buf(kind, nxt)
            d.step_eval_observe_dev(calls[2].e, od["done"].ptr, od["lines"].ptr, od["dead"].ptr, nb.ptr, obs["visual"].ptr, obs["vector"].ptr,
                                    obs["piece"].ptr, auto_reset=True)
        done = o.step_rt(want["rot"], want["trans"], player)
        rec = o.observe()[0]
        finished = np.nonzero(done)[0].astype(np.int32)
        ended += len(finished)
        for call, out, name in ((calls[0], oa, "step_eval_dev"), (calls[1], oc, "select_eval_dev + step_rt_dev")) + (((calls[2], od, "step_eval_observe_dev"),) if observe else ()):
            assert_outputs(call.get(), want, f"step {s} ({mode}): {name}")
            assert np.array_equal(out["done"].get(), done), f"step {s}: {name} 'done'"
            assert np.array_equal(out["lines"].get(), rec["reward"].T) and np.array_equal(out["dead"].get(), rec["dead"].T), f"step {s}: {name} lines / dead"
        if len(finished):
            episode[finished] += 1
            o.reset(finished, seeds=orc.episode_seed(ids[finished], episode[finished]))
        engines.assert_same_state(a, o, where=f"step {s}: step_eval_dev against the oracle")
        engines.assert_same_state(c, a, where=f"step {s}: select_eval_dev + step_rt_dev against step_eval_dev")
        if observe:
            engines.assert_same_state(d, a, where=f"step {s}: step_eval_observe_dev against step_eval_dev")
            for got, want_obs, name in zip((obs["visual"].get(), obs["vector"].get(), obs["piece"].get()), a.observe_packed(player=nxt), ("visual", "vector", "piece")):
                assert np.array_equal(got, want_obs), f"step {s}: step_eval_observe_dev '{name}'"
    assert ended > 0, "no game finished: auto-reset is not inside the comparison"
    assert a.take_errors() == 0 and c.take_errors() == 0 and d.take_errors() == 0


# ---------------------------------------------------------------- 6. arguments
def test_arguments_are_checked():
    pkg = ge.package()
    n = 4
    b, o = midgame("harness", n, 2, steps=3)
    ae = np.zeros((n, 4, 10, 7), F32)
    se = np.zeros((n, 7), F32)
    rot, trans, value, ent = np.full(n, 9, np.uint8), np.full(n, 9, np.uint8), np.zeros((2, n), F32), np.zeros(n, F32)
    p = lambda arr: arr.ctypes.data                                                           # noqa: E731
    good = dict(n_pieces=7, mode="argmax")
    bad = [
        (dict(action_eval=None), "NULL"),
        (dict(rot=None), "NULL"),
        (dict(trans=None), "NULL"),
        (dict(n_pieces=5), "n_pieces"),
        (dict(n_pieces=0), "n_pieces"),
        (dict(state_eval=p(se), n_values=5), "n_values"),
        (dict(value=p(value)), "state_eval"),
        (dict(mode=4), "mode"),
        (dict(mode=-1), "mode"),
        (dict(flags=4), "flag"),
        (dict(mode="rank"), "table"),
        (dict(mode="argmax", entropy=p(ent)), "entropy"),
        (dict(action_eval=p(ae) + 4), "aligned"),
    ]
    for kw, text in bad:
        args = dict(action_eval=p(ae), rot=p(rot), trans=p(trans))
        args.update(good)
        args.update(kw)
        e = b.act_eval(args.pop("action_eval"), args.pop("rot"), args.pop("trans"), **args)
        for call in (lambda: b.select_eval_dev(e), lambda: b.step_eval_dev(e, None, None, None),
                     lambda: b.step_eval_observe_dev(e, None, None, None, None, p(np.zeros((2, n, 20, 10), np.uint8)), p(np.zeros((2, n, 12), np.uint8)), p(np.zeros((2, n), np.uint8)))):
            with pytest.raises(pkg.TetrisError, match=text):
                call()
    e = b.act_eval(p(ae), p(rot), p(trans))
    for call in (lambda: b.select_eval_dev(None), lambda: b.step_eval_dev(None, None, None, None)):
        with pytest.raises(pkg.TetrisError, match="NULL"):
            call()
    assert b.lib.tetris_step_eval_dev(b._h, __import__("ctypes").byref(e), 400, 2, None, None, None) == -1 and b"flag" in b.lib.tetris_last_error()
    with pytest.raises(pkg.TetrisError, match="NULL"):
        b.step_eval_observe_dev(e, None, None, None, None, None, None, None)
    s = pkg.TetrisBatch(n, 2, 20, 10, lib_path=ge.build_harness(), split_side=0)
    for call in (lambda: s.select_eval_dev(e), lambda: s.step_eval_dev(e, None, None, None)):
        with pytest.raises(pkg.TetrisError, match="split"):
            call()
    three = engines.make("harness", n, 3)
    with pytest.raises(pkg.TetrisError, match="one or two players"):
        three.step_eval_observe_dev(e, None, None, None, None, p(np.zeros((3, n, 20, 10), np.uint8)), p(np.zeros((3, n, 12), np.uint8)), p(np.zeros((3, n), np.uint8)))
    assert np.all(rot == 9) and np.all(trans == 9), "a rejected call must not run"
    engines.assert_same_state(b, o, where="a rejected call must not run")
    assert pkg.ACT_MODES == dict(argmax=0, pi=1, rank=2, epsilon=3)


def test_host_entropies_restate_the_reference():
    """The entropies that do not depend on the map (TorchEnv returns them as Python floats): sventon_utils.py:21-45."""
    capi = ge.package().capi
    assert capi.act_entropy("argmax") == 0.0
    p = np.full(40, 0.3 / 40)
    p[0] += 0.7
    assert capi.act_entropy("epsilon", epsilon=0.3) == pytest.approx(-np.sum(p * np.log(p + 1e-8)), abs=1e-12)
    assert capi.act_entropy("epsilon", epsilon=5.0) == pytest.approx(np.log(40), abs=1e-6)
    t = np.arange(1, 41) ** -1.5
    assert capi.act_entropy("rank", table=capi.pareto_table(1.5)) == pytest.approx(-np.sum(t / t.sum() * np.log(t / t.sum() + 1e-8)), abs=1e-6)
    assert np.array_equal(capi.pareto_table(1.0), pareto(1.0))


# ---------------------------------------------------------------- 7. torch interface
def _fake_network(visual, vector, K=7):
    """a fixed function of the observation, float32 [n, 4, 10, K] and [n, K]; the same arithmetic in numpy and in torch (integer
    sums, then one float32 division: no reduction order enters)"""
    xp = np if isinstance(visual, np.ndarray) else __import__("torch")
    n = visual.shape[1]
    if xp is np:
        heights = visual[0].astype(np.int64).sum(axis=1)                                   # [n, 10]
        rt = np.arange(40, dtype=np.int64).reshape(1, 4, 10, 1)
        k = np.arange(K, dtype=np.int64).reshape(1, 1, 1, K)
        x, y = vector[0][:, 0].astype(np.int64).reshape(n, 1, 1, 1), vector[0][:, 1].astype(np.int64).reshape(n, 1, 1, 1)
        mix = (heights.reshape(n, 1, 10, 1) * 7 + rt * 13 + k * 29 + x * 3 + y * 5 + heights.sum(axis=1).reshape(n, 1, 1, 1)) % 31
        return (mix.astype(np.float32) / np.float32(8.0)).astype(np.float32), ((mix[:, 0, 0, :] % 9).astype(np.float32) / np.float32(4.0)).astype(np.float32)
    heights = visual[0].to(xp.int64).sum(dim=1)
    rt = xp.arange(40, dtype=xp.int64, device=visual.device).view(1, 4, 10, 1)
    k = xp.arange(K, dtype=xp.int64, device=visual.device).view(1, 1, 1, K)
    x, y = vector[0][:, 0].to(xp.int64).view(n, 1, 1, 1), vector[0][:, 1].to(xp.int64).view(n, 1, 1, 1)
    mix = (heights.view(n, 1, 10, 1) * 7 + rt * 13 + k * 29 + x * 3 + y * 5 + heights.sum(dim=1).view(n, 1, 1, 1)) % 31
    return (mix.to(xp.float32) / 8.0).contiguous(), ((mix[:, 0, 0, :] % 9).to(xp.float32) / 4.0).contiguous()


@pytest.mark.gpu
def test_torch_env_calls_equal_the_c_level_results():
    import importlib
    import torch
    ti = importlib.import_module("drl-tetris_amd.torch_interop")
    n, P = 130, 2
    rng = np.random.default_rng(70)
    a, c, o = midgame("hip", n, P, extra=1)
    te = ti.TorchEnv(a)
    player = rng.integers(0, P, n).astype(np.uint8)
    pt = torch.from_numpy(player).cuda()
    for dtype, tdt in ((np.float32, torch.float32), (np.float16, torch.float16)):
        ae = random_maps(rng, n, 7, dtype, "pi")
        se = rng.standard_normal((n, 8)).astype(dtype)
        at = torch.from_numpy(ae.view(np.int16) if dtype == np.float16 else ae).cuda().view(tdt)
        st = torch.from_numpy(se.view(np.int16) if dtype == np.float16 else se).cuda().view(tdt)
        for draw, mode in enumerate(MODES):
            kw = dict(seed=21, draw=draw, epsilon=0.4)
            call = Call("hip", c, ae, mode, player=player, state_eval=se, table=pareto(0.7) if mode == "rank" else None, **kw)
            c.select_eval_dev(call.e)
            want = call.get()
            rot, trans, piece, ev, value, entropy = te.select_eval(at, st, mode=mode, player=pt, theta=0.7 if mode == "rank" else None, **kw)
            got = dict(rot=rot.cpu().numpy(), trans=trans.cpu().numpy(), piece=piece.cpu().numpy(), eval=ev.cpu().numpy(), value=value.cpu().numpy())
            assert_outputs(got, want, f"TorchEnv.select_eval {mode}")
            assert_outputs(got, model(ae, pieces_of(o, player), np.arange(n), mode, state_eval=se, table=pareto(0.7), **kw), f"TorchEnv.select_eval {mode} against the model")
            if mode == "pi":
                assert np.array_equal(bits(entropy.cpu().numpy()), bits(want["entropy"]))
            else:
                assert isinstance(entropy, float)
    # step_eval / step_eval_observe against the C-level calls on the copy
    ae = random_maps(rng, n, 7, np.float32, "normal")
    at = torch.from_numpy(ae).cuda()
    done, lines, dead = (Buf("hip", np.zeros(s, np.uint8)) for s in ((n,), (P, n), (P, n)))
    for draw, fused in enumerate((False, True)):
        call = Call("hip", c, ae, "pi", player=player, seed=4, draw=draw)
        c.step_eval_dev(call.e, done.ptr, lines.ptr, dead.ptr, auto_reset=True)
        if fused:
            out = te.step_eval_observe(at, mode="pi", player=pt, next_player=pt, seed=4, draw=draw, auto_reset=True)
            vis, vec, pc = c.observe_packed(player=player)
            assert np.array_equal(out[3].cpu().numpy(), vis) and np.array_equal(out[4].cpu().numpy(), vec) and np.array_equal(out[5].cpu().numpy(), pc)
            rot, trans = out[6], out[7]
        else:
            out = te.step_eval(at, mode="pi", player=pt, seed=4, draw=draw, auto_reset=True)
            rot, trans = out[3], out[4]
        want = call.get()
        assert np.array_equal(rot.cpu().numpy(), want["rot"]) and np.array_equal(trans.cpu().numpy(), want["trans"])
        assert np.array_equal(out[0].cpu().numpy(), done.get()) and np.array_equal(out[1].cpu().numpy(), lines.get())
        torch.cuda.synchronize()
        engines.assert_same_state(a, c, where="TorchEnv step against the C-level call")


@pytest.mark.gpu
def test_torch_agent_loop_equals_the_oracle_and_the_model():
    """observe -> fake network -> step_eval_observe, 20 iterations, nothing synchronised inside the loop; then the same loop on
    the oracle with the numpy model.  (The oracle has no packed observation: its inputs are rebuilt from its records.)"""
    import importlib
    import torch
    ti = importlib.import_module("drl-tetris_amd.torch_interop")
    n, P, iters = 96, 2, 20
    a, o = midgame("hip", n, P)
    te = ti.TorchEnv(a)
    players = [torch.full((n,), s % P, dtype=torch.uint8, device="cuda") for s in range(2)]
    visual, vector, _ = te.observe(players[0])
    history = []
    for s in range(iters):
        at, st = _fake_network(visual, vector)
        out = te.step_eval_observe(at, st, mode=MODES[s % 4], player=players[s % 2], next_player=players[(s + 1) % 2], seed=31, draw=s,
                                   epsilon=0.5, theta=1.0 if MODES[s % 4] == "rank" else None, auto_reset=True)
        visual, vector = out[3], out[4]
        history.append([t.clone() for t in (out[0], out[6], out[7], out[8], out[9], out[10][0], out[10][1])])
    torch.cuda.synchronize()
    history = [[t.cpu().numpy() for t in h] for h in history]
    ids, episode = np.arange(n), np.zeros(n, np.int64)
    ended = 0
    for s in range(iters):
        me = s % P
        rec = o.observe()[0]
        vis = np.stack([(rec["field"][:, p, :20, :] > 0).astype(np.uint8) for p in (me, 1 - me)])
        vec = np.zeros((2, n, 12), np.uint8)
        vec[0, :, 0], vec[0, :, 1] = rec["x"][:, me].astype(np.uint8), rec["y"][:, me].astype(np.uint8)
        ae, se = _fake_network(vis, vec)
        want = model(ae, rec["piece"][:, me], ids, MODES[s % 4], seed=31, draw=s, epsilon=0.5, table=pareto(1.0), state_eval=se)
        done_g, rot, trans, piece, ev, v0, v1 = history[s]
        assert_outputs(dict(rot=rot, trans=trans, piece=piece, eval=ev, value=np.stack([v0, v1])), want, f"iteration {s}")
        done = o.step_rt(want["rot"], want["trans"], np.full(n, me, np.uint8))
        assert np.array_equal(done_g, done), f"iteration {s}: done"
        finished = np.nonzero(done)[0].astype(np.int32)
        ended += len(finished)
        if len(finished):
            episode[finished] += 1
            o.reset(finished, seeds=orc.episode_seed(ids[finished], episode[finished]))
    engines.assert_same_state(a, o, where="the agent loop")
    assert a.take_errors() == 0
