"""Choosing a planning agent's action list on the device from phi (include/tetris_hip.h: tetris_select_lists_dev,
tetris_step_lists_eval_dev) against a model written here from the header's definitions — numpy float32, every sum an explicit
sequential loop in the stated order (a score's loop runs over cells in that order and is vectorised over the lists only),
oracle.philox for the words — on columns the tests craft themselves, against tetris_plan_deltas_dev for the two planes, against
the reference's arithmetic in float64 (sherlock_agent.py:101-109), against the oracle for the step and, on the MI355X, against the
torch composition the call replaces.  The tests parametrised over engines.ENGINE_PARAMS run on the CPU harness (`-m "not gpu"`) and
on the GPU (`-m gpu`); on the harness the "device" buffers are numpy arrays."""
import ctypes
import importlib

import numpy as np
import pytest

import __graft_entry__ as ge
from oracle import oracle as orc
from tests import engines
from tests.act_support import midgame, pieces_of, unit, words
from tests.buffers import Buf, bits, out
from tests.plan_support import Call, _crafted, _device_lists, _numpy_deltas, _plan_env, _run, _simulate, _words, crafted_phi

F32 = np.float32
MODES = ("argmax", "pi")


# ---------------------------------------------------------------- the model
def model_scores(phi, piece_idx, before, after, count, fill):
    """phi [N, H, 10, K] (float32 or float16), piece_idx [N] (observe()'s `piece` of the acting players), before bool [N, H, 10],
    after bool [N, L, H, 10], count int [N] -> (piece [N], cnt [N], kind [N, L] (0 normal, 1 small, 2 past), score float32 [N, L])"""
    N, L, H = after.shape[:3]
    K = phi.shape[3]
    piece = np.minimum(piece_idx, K - 1).astype(np.uint8)
    cnt = np.clip(count, 0, L)
    delta = after.astype(np.int32) - before[:, None].astype(np.int32)
    valid = np.arange(L)[None, :] < cnt[:, None]
    small = valid & (delta.sum(axis=(2, 3)) < 4)
    kind = np.where(~valid, 2, np.where(small, 1, 0))
    score = np.zeros((N, L), F32)
    with np.errstate(all="ignore"):
        for i in range(N):
            w = phi[i, :, :, piece[i]].astype(F32)
            s = np.zeros(L, F32)
            plane = None
            for c in range(10):
                col = F32(0.0)
                for y in range(H):
                    col = F32(col + w[y, c])
                    d = delta[i, :, y, c]
                    s = np.where(d > 0, s + w[y, c], np.where(d < 0, s - w[y, c], s)).astype(F32)
                plane = col if c == 0 else F32(plane + col)
            score[i] = np.where(kind[i] == 0, s, np.where(kind[i] == 1, F32(F32(fill) * plane), F32(0.0)))
    return piece, cnt, kind, score


def model(phi, piece_idx, before, after, count, fill, mode, ids=None, seed=0, draw=0, state_eval=None, scores=None):
    """-> dict of choice, piece, prob, probs [N, L], entropy (float64), value [2, N], delta [N, H, 10], sums [N, H, 10] and the model's own kind, cnt, degenerate, fell_back"""
    N, L, H = after.shape[:3]
    piece, cnt, kind, score = scores if scores is not None else model_scores(phi, piece_idx, before, after, count, fill)
    ids = np.arange(N) if ids is None else ids
    w4 = words(seed, ids, draw) if mode == "pi" else np.zeros((N, 4), np.uint32)
    choice, prob, probs, entropy = np.zeros(N, np.int32), np.zeros(N, F32), np.zeros((N, L), F32), np.zeros(N, np.float64)
    degenerate, fell_back = np.zeros(N, bool), np.zeros(N, bool)
    with np.errstate(all="ignore"):
        for i in range(N):
            c = int(cnt[i])
            if c == 0:
                continue
            total = F32(0.0)
            for k in range(c):
                total = F32(total + score[i, k])
            q = (score[i, :c] / total).astype(F32)
            probs[i, :c] = q
            if np.isnan(q).any():
                degenerate[i] = True
                prob[i] = q[0]
                continue
            pick = int(np.argmax(q))                               # numpy's first maximum is the lowest list
            if mode == "pi":
                m = np.where(q > 0, q, F32(0.0)).astype(F32)
                run, partial = F32(0.0), []
                for k in range(c):
                    run = F32(run + m[k])
                    partial.append(run)
                if run > 0 and np.isfinite(run):
                    target = F32(unit(w4[i, 0]) * run)
                    over = [k for k in range(c) if partial[k] > target]
                    pick = over[0] if over else int(np.nonzero(m > 0)[0][-1])
                else:
                    fell_back[i] = True
                q64 = q.astype(np.float64)
                entropy[i] = -(q64 * np.log(q64 + 1e-8)).sum()
            choice[i], prob[i] = pick, q[pick]
    delta = after.astype(np.int32) - before[:, None].astype(np.int32)
    ck = kind[np.arange(N), choice]
    dplane = np.where((ck == 0)[:, None, None], delta[np.arange(N), choice], 0).astype(F32)
    dplane[ck == 1] = F32(fill)
    dplane[cnt == 0] = 0.0
    isum = np.where((kind == 0)[:, :, None, None], delta, 0).sum(axis=1)
    sums = isum.astype(F32) + (F32(fill) * (kind == 1).sum(axis=1).astype(F32))[:, None, None]
    out = dict(choice=choice, piece=piece, prob=prob, probs=probs, entropy=entropy, delta=dplane, sums=sums.astype(F32), kind=kind, cnt=cnt,
               degenerate=degenerate, fell_back=fell_back)
    if state_eval is not None:
        V = state_eval.shape[1]
        se = state_eval.astype(F32)
        mean = np.zeros(N, F32)
        for k in range(V):
            mean = (mean + se[:, k]).astype(F32)
        out["value"] = np.stack([se[np.arange(N), np.minimum(piece, V - 1)] if V > 1 else se[:, 0], (mean / F32(V)).astype(F32)])
    return out


def assert_outputs(got, want, where, planes=True):
    for name in ("choice", "piece"):
        assert np.array_equal(got[name], want[name]), f"{where}: '{name}' differs in games {np.nonzero(got[name] != want[name])[0][:8]}"
    for name in ("prob", "probs", "value") + (("delta", "sums") if planes else ()):
        if name in got:
            assert np.array_equal(bits(got[name]), bits(want[name])), f"{where}: '{name}' differs"
    cnt = want["cnt"]
    assert (got["choice"] >= 0).all() and (got["choice"] < np.maximum(cnt, 1)).all(), f"{where}: a choice outside [0, max(count, 1))"


def assert_entropy(got, want, where):
    """as test_act_eval.test_entropy_of_pi: against the formula in float64, absolute tolerance 5e-5, on the games whose q are a
    probability map (all q >= 0; they add up to 1); elsewhere (a log of a negative number) both sides are NaN or neither is"""
    q_ok = (want["probs"] >= 0).all(axis=1) & ~want["degenerate"] & (want["cnt"] > 0)
    err = np.abs(got["entropy"].astype(np.float64) - want["entropy"])
    print(f"{where}: entropy on {q_ok.sum()} games, largest error {err[q_ok].max() if q_ok.any() else 0:.3g}")
    assert (err[q_ok] < 5e-5).all(), where
    assert np.array_equal(np.isnan(got["entropy"]), np.isnan(want["entropy"])), where
    assert (got["entropy"][want["degenerate"] | (want["cnt"] == 0)] == 0).all(), where
    return int(q_ok.sum())


# ---------------------------------------------------------------- 1. the model on crafted columns
_CRAFTED = {}


@pytest.fixture(scope="module", autouse=True)
def _close_crafted_batches():
    """the crafted batches are shared by the cases of this module and closed with it: a batch left open keeps its stream, and
    with it a place on one of the device's few hardware queues, for every test file that runs afterwards"""
    yield
    for case in _CRAFTED.values():
        case[0].close()
    _CRAFTED.clear()


def _crafted_case(kind, P, H, L):
    """the crafted batch of one shape and the planes of tetris_plan_deltas_dev on it, made once per engine"""
    key = (kind, P, H, L)
    if key not in _CRAFTED:
        N, fill = 67, 1e-3
        b, player, count, cols, before, after = _crafted(kind, N, P, H, L, seed=100 * P + H + L)
        who = np.minimum(player, P - 1)
        d, s, _ = _run(kind, b, player, count, cols, L, fill)
        dh, sh, _ = _run(kind, b, player, count, cols, L, fill, f16=True)
        _CRAFTED[key] = (b, player, count, cols, before, after, pieces_of(b, who), (d, s, dh, sh), {})
    return _CRAFTED[key]


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", [np.float32, np.float16], ids=["float32", "float16"])
@pytest.mark.parametrize("K", [1, 7])
@pytest.mark.parametrize("P,H,L", [(1, 20, 7), (2, 20, 64), (2, 7, 1), (4, 31, 130), (1, 31, 256), (2, 20, 256)])
def test_crafted_columns_match_the_model(kind, P, H, L, K, dtype, mode):
    """The first four shapes take the kernel's 32-games-per-workgroup form, the two with 256 lists its 16-game form
    (tetris_choose.h: choose_games_per_block — from 138 lists at 31 rows, from 226 at 20)."""
    N, fill = 67, 1e-3
    assert _games_per_block(H, L) == (16 if L == 256 else 32)
    b, player, count, cols, before, after, piece_idx, (d, s, dh, sh), cache = _crafted_case(kind, P, H, L)
    rng = np.random.default_rng(7 * P + H + L + K)
    phi = crafted_phi(rng, N, H, K, dtype)
    V = (7, 8, 1)[(L + K) % 3]
    state_eval = rng.standard_normal((N, V)).astype(dtype)
    if (K, dtype) not in cache:
        cache[(K, dtype)] = model_scores(phi, piece_idx, before, after, count, fill)
    want = model(phi, piece_idx, before, after, count, fill, mode, seed=77, draw=L, state_eval=state_eval, scores=cache[(K, dtype)])
    # the inputs hold every kind of list, every edge of count, out-of-range players and negative deltas
    knd = want["kind"]
    assert (knd == 0).sum() > 0 and (knd == 1).sum() > 0 and (knd == 2).sum() > 0
    assert {-1, 0, L, L + 5} <= set(count.tolist()) and (player >= P).sum() > 0
    assert ((after.astype(np.int32) - before[:, None].astype(np.int32))[knd == 0] < 0).sum() > 0
    if H == 20 and K == 7:
        assert len(np.unique(want["piece"])) > 1
    blob = b.snapshot()
    call = Call(kind, b, phi, player, count, cols, L, mode, fill=fill, state_eval=state_eval, seed=77, draw=L)
    b.select_lists_dev(call.e)
    got = call.get()
    assert_outputs(got, want, f"{mode}")
    if mode == "pi":
        assert_entropy(got, want, "pi")
    # the two planes are those of tetris_plan_deltas_dev on the same inputs, in both element types
    pick = np.where(want["cnt"] > 0, got["choice"], 0)
    plane = d[np.arange(N), :, :, pick]
    plane[want["cnt"] == 0] = 0.0
    assert np.array_equal(bits(got["delta"]), bits(plane)) and np.array_equal(bits(got["sums"]), bits(s))
    half = Call(kind, b, phi, player, count, cols, L, mode, fill=fill, seed=77, draw=L, out_f16=True)
    b.select_lists_dev(half.e)
    goth = half.get()
    plane = dh[np.arange(N), :, :, pick]
    plane[want["cnt"] == 0] = 0.0
    assert np.array_equal(goth["choice"], got["choice"])
    assert np.array_equal(goth["delta"].view(np.uint16), plane.view(np.uint16)) and np.array_equal(goth["sums"].view(np.uint16), sh.view(np.uint16))
    assert np.array_equal(b.snapshot(), blob), "the batch's state was written"
    assert b.take_errors() == 0


def _games_per_block(H, L):
    """tetris_choose.h's sizing restated: 32 games per workgroup where their LDS image fits 64 KB, else 16"""
    return 32 if ((H * 10 + L + 10) * 33 + 6 * 32) * 4 + L * 32 <= 65536 else 16


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("mode", MODES)
def test_a_cell_that_256_lists_fill(kind, mode):
    """19 one-player games (two workgroups of the 16-game form, the second partial) with 256, 255 or 254 lists, every one normal:
    four cells that all of a game's lists fill — the sums there are the list count, 256 included, which takes the ninth bit of the
    kernel's per-cell counters — and one more cell that goes round with the list number."""
    N, L, H = 19, 256, 20
    assert _games_per_block(H, L) == 16
    b, before, after = _own_lists(kind, N, L, H)
    rng = np.random.default_rng(256)
    count = (L - np.arange(N) % 3).astype(np.int32)
    for i in range(N):
        cells = rng.permutation(H * 10)[:11]
        for k in range(L):
            after[i, k].reshape(-1)[cells[:4]] = True
            after[i, k].reshape(-1)[cells[4 + k % 7]] = True
    phi = (rng.random((N, H, 10, 1)) + 0.5).astype(F32)
    want = model(phi, np.zeros(N, np.int64), before, after, count, 1e-3, mode, seed=3, draw=2)
    assert (want["kind"][np.arange(L)[None, :] < count[:, None]] == 0).all()
    assert (want["sums"].max(axis=(1, 2)) == count).all() and want["sums"].max() == 256
    call = Call(kind, b, phi, None, count, _cols_of(after), L, mode, seed=3, draw=2)
    b.select_lists_dev(call.e)
    got = call.get()
    assert_outputs(got, want, f"256 lists, {mode}")
    if mode == "pi":
        assert assert_entropy(got, want, "256 lists") == N
    assert b.take_errors() == 0


# ---------------------------------------------------------------- 2. the degenerate rules
def _own_lists(kind, N, L, H=20, seed=1):
    """one-player games on empty boards, lists the test fills cell by cell: -> (b, after bool [N, L, H, 10])"""
    b = engines.make(kind, N, 1, height=H, seeds=orc.episode_seed(np.arange(N), seed))
    before = b.observe()[0]["field"][:, 0, :H] > 0
    assert not before.any()
    return b, before, np.zeros((N, L, H, 10), bool)


def _cols_of(after):
    """after bool [N, L, H, 10] of one-player games -> d_cols uint32 [L, 1, 10, N]"""
    return np.ascontiguousarray(_words(after).transpose(1, 2, 0)[:, None])


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("mode", MODES)
def test_degenerate_rules(kind, mode):
    """game 0: all-zero phi (total 0, every q NaN); 1: a NaN in phi under a stamped cell; 2: negative phi, a negative total — the
    argmax follows q, not the scores; 3: scores 1e20, -1e20, 1e-20: q = inf, -inf, 1, sum(m) = inf — PI falls back to ARGMAX;
    4: two scores of 3e38, total inf, every q 0, sum(m) = 0 — PI falls back to ARGMAX; 5: count 0; 6: an ordinary game.
    The boards hold one cell (7, 0) that a list of game 3 removes."""
    N, L, H = 7, 4, 20
    b = engines.make(kind, N, 1, height=H, seeds=orc.episode_seed(np.arange(N), 3))
    # a cell to take away: the games are stepped once so that a piece lies on the floor
    b.step_rt(np.zeros(N, np.uint8), np.zeros(N, np.uint8))
    before = b.observe()[0]["field"][:, 0, :H] > 0
    assert before.any(axis=(1, 2)).all()
    after = np.repeat(before[:, None], L, axis=1)
    free = [np.argwhere(~before[i]) for i in range(N)]
    used = [np.argwhere(before[i]) for i in range(N)]
    for i in range(N):
        for k in range(L):
            for y, x in free[i][5 * k: 5 * k + 4 + (k % 2)]:           # 4 or 5 new cells: a normal list
                after[i, k, y, x] = True
    phi = np.full((N, H, 10, 1), 0.25, F32)
    phi[0] = 0.0
    phi[1, free[1][2][0], free[1][2][1], 0] = np.nan                    # under a cell of list 0
    phi[2] = -np.linspace(0.5, 1.5, H * 10, dtype=F32).reshape(H, 10, 1)
    # game 3: list 0 adds four cells of 0 and one of 1e20; list 1 removes a cell of 1e20 and adds five of 0; list 2 adds 1e-20 x 4 ...
    phi[3] = 0.0
    after[3] = before[3]
    f3, u3 = free[3], used[3]
    for y, x in f3[0:5]:
        after[3, 0, y, x] = True
    phi[3, f3[0][0], f3[0][1], 0] = 1e20
    after[3, 1, u3[0][0], u3[0][1]] = False
    phi[3, u3[0][0], u3[0][1], 0] = 1e20
    for y, x in f3[5:10]:
        after[3, 1, y, x] = True
    for y, x in f3[10:14]:
        after[3, 2, y, x] = True
    phi[3, f3[10][0], f3[10][1], 0] = 1e-20
    phi[4] = 0.0
    for k in range(2):                                                  # (lists 2 and 3 of game 4 score 0)
        y, x = free[4][5 * k]
        phi[4, y, x, 0] = 3e38
    count = np.array([L, L, L, 3, L, 0, L], np.int32)
    cols = _cols_of(after)
    piece_idx = pieces_of(b, np.zeros(N, np.int64))
    want = model(phi, piece_idx, before, after, count, 0.0, mode, seed=5, draw=1)
    # the cases are what the docstring says
    assert want["degenerate"].tolist() == [True, True, False, False, False, False, False]
    assert np.isnan(want["probs"][0, :L]).all() and np.isnan(want["probs"][1]).any()
    assert (want["probs"][2] > 0).all()
    assert np.isposinf(want["probs"][3, 0]) and np.isneginf(want["probs"][3, 1]) and want["probs"][3, 2] == 1.0
    assert (want["probs"][4] == 0).all()
    if mode == "pi":
        assert want["fell_back"].tolist() == [False, False, False, True, True, False, False]
    assert want["choice"][:2].tolist() == [0, 0] and want["choice"][3] == 0 and want["choice"][4] == 0 and want["choice"][5] == 0
    call = Call(kind, b, phi, None, count, cols, L, mode, fill=0.0, seed=5, draw=1)
    b.select_lists_dev(call.e)
    got = call.get()
    assert_outputs(got, want, f"degenerate, {mode}")
    # argmax on negative phi: the chosen list has the highest q, which is the LOWEST (most negative) score
    _, _, _, score = model_scores(phi, piece_idx, before, after, count, 0.0)
    assert (score[2] < 0).all() and model(phi, piece_idx, before, after, count, 0.0, "argmax")["choice"][2] == int(np.argmin(score[2]))
    if mode == "pi":
        assert (got["entropy"][[0, 1, 5]] == 0).all()
    assert got["prob"][5] == 0 and not got["delta"][5].any() and not got["probs"][5].any()
    assert b.take_errors() == 0


# ---------------------------------------------------------------- 3. the draw
def _draw_inputs(kind, N=6, L=8, H=20):
    b, before, after = _own_lists(kind, N, L, H)
    rng = np.random.default_rng(11)
    for i in range(N):
        for k in range(L):
            cells = rng.permutation(H * 10)[: (3 if (i + k) % 4 == 3 else 4 + k % 3)]      # three cells: a small list, q = 0
            after[i, k].reshape(-1)[cells] = True
    phi = (rng.random((N, H, 10, 1)) + 0.5).astype(F32)
    return b, before, after, phi, np.full(N, L, np.int32)


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
def test_the_draw_is_keyed_by_seed_game_and_draw(kind):
    N, L = 6, 8
    b, before, after, phi, count = _draw_inputs(kind)
    cols = _cols_of(after)
    zero = np.zeros(N, np.int64)
    scores = model_scores(phi, zero, before, after, count, 0.0)

    def run(**kw):
        call = Call(kind, b, phi, None, count, cols, L, "pi", fill=0.0, small_outputs_only=True, **kw)
        b.select_lists_dev(call.e)
        return call.get()["choice"]

    def want(ids, **kw):
        return model(phi, zero, before, after, count, 0.0, "pi", ids=ids, scores=scores, **kw)["choice"]

    first = run(seed=1, draw=5)
    assert np.array_equal(first, want(np.arange(N), seed=1, draw=5))
    assert np.array_equal(run(seed=1, draw=5), first), "the same (seed, draw) must repeat its choices"
    others = [run(seed=1, draw=6), run(seed=2, draw=5), run(seed=1, draw=5 + (1 << 32))]
    for got, kw in zip(others, (dict(seed=1, draw=6), dict(seed=2, draw=5), dict(seed=1, draw=5 + (1 << 32)))):
        assert np.array_equal(got, want(np.arange(N), **kw))
        assert (got != first).any(), f"{kw} must change the choices"
    b.set_game_offset(7)
    shifted = run(seed=1, draw=5)
    assert np.array_equal(shifted, want(np.arange(N) + 7, seed=1, draw=5)) and (shifted != first).any()


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
def test_distribution_of_the_draw(kind):
    """One fixed phi, 4 096 draw numbers, six games: every list with q > 0 is reached, none with q = 0, and every list's count is
    within 5 standard deviations of a binomial with 4 096 draws and probability q.  The seed is fixed: the test is deterministic."""
    N, L, D = 6, 8, 4096
    b, before, after, phi, count = _draw_inputs(kind)
    cols = _cols_of(after)
    q = model(phi, np.zeros(N, np.int64), before, after, count, 0.0, "argmax")["probs"].astype(np.float64)
    assert (q == 0).sum() >= N and ((q > 0).sum(axis=1) >= 5).all()
    choices = out(kind, (D, N), np.int32)
    base = Call(kind, b, phi, None, count, cols, L, "pi", fill=0.0, small_outputs_only=True, entropy=False)
    for draw in range(D):                                                  # every draw writes its own row: one read-back at the end
        base.e.draw = draw
        base.e.d_choice = choices.ptr + 4 * N * draw
        b.select_lists_dev(base.e)
    got = choices.get()
    for i in range(N):
        n_k = np.bincount(got[:, i], minlength=L)
        sd = np.sqrt(D * q[i] * (1 - q[i]))
        print(f"game {i}: counts {n_k.tolist()}, expected {np.round(D * q[i], 1).tolist()}, deviations in sd {np.round((n_k - D * q[i]) / np.maximum(sd, 1e-9), 2).tolist()}")
        assert n_k.sum() == D and ((n_k > 0) == (q[i] > 0)).all()
        assert (np.abs(n_k - D * q[i]) <= 5 * sd).all()


# ---------------------------------------------------------------- 4. the reference's arithmetic
def _reference_probs(d64, phi, piece):
    """sherlock_agent.py:101-109 in float64 over deltas [n, H, 10, L]; phi [n, H, 10, K] -> probabilities [n, L]"""
    n = d64.shape[0]
    phi_p = phi.astype(np.float64)[np.arange(n), :, :, piece][..., None]
    p_unnormalized = (d64 * phi_p).sum(axis=(1, 2))
    return p_unnormalized / p_unnormalized.sum(axis=1, keepdims=True)


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("dtype", [np.float32, np.float16], ids=["float32", "float16"])
def test_probabilities_match_the_reference_arithmetic(kind, dtype):
    """Strictly positive phi, small_fill = 0 (the reference's uint8 fields), mid-game boards: relative tolerance
    2 (H + L + 12) 2^-24 — at most H + 9 roundings in a score, L - 1 in the total, one division, all terms positive."""
    n, L, H = 64, 64, 20
    env = _plan_env(kind, n)
    b = env.backend
    player = np.arange(n) % 2
    cnt, lens, keys, pl = _device_lists(kind, b, player, False, L=L)
    cols = _simulate(kind, b, cnt, lens, keys, pl, False, L=L)[0]
    rng = np.random.default_rng(3)
    phi = (rng.random((n, H, 10, 7)) + 0.1).astype(dtype)
    call = Call(kind, b, phi, player, cnt.get(), cols, L, "argmax", fill=0.0)
    b.select_lists_dev(call.e)
    got = call.get()
    d64, _ = _numpy_deltas(env.get_state(), env.simulate_all_actions(player=player.tolist(), finalize=False), player, L)
    small = (d64 == 1e-3).all(axis=(1, 2))                                  # [n, L]: np.full_like on the uint8 field gives 0
    d64 = np.where(small[:, None, None, :], 0.0, d64)
    piece = pieces_of(b, player)
    assert np.array_equal(got["piece"], piece)
    want = _reference_probs(d64, phi, piece)
    tol = 2 * (H + L + 12) * 2.0 ** -24
    rel = np.abs(got["probs"].astype(np.float64) - want) / np.maximum(want, 1e-300)
    print(f"probs: largest relative error {rel[want > 0].max():.3g} (tolerance {tol:.3g})")
    assert (want >= 0).all() and (rel[want > 0] <= tol).all() and (got["probs"][want == 0] == 0).all()
    assert np.array_equal(got["choice"], got["probs"].argmax(axis=1))
    assert b.take_errors() == 0


# ---------------------------------------------------------------- 5. the step
@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("auto", [False, True], ids=["plain", "auto_reset"])
@pytest.mark.parametrize("P", [1, 2])
def test_step_equals_select_plus_step_lists_and_the_oracle(kind, P, auto):
    """24 decisions at 64 games, the two modes in turn: tetris_step_lists_eval_dev against tetris_select_lists_dev +
    tetris_step_lists_dev on a copy (every output, every state word), and against the oracle stepping the chosen key list.  With
    auto-reset the oracle resets finished games by the built-in seed schedule; without, finished games stay as they ended."""
    n, L, K, steps = 64, 64, 48, 24
    a, c, o = midgame(kind, n, P, extra=1)
    rng = np.random.default_rng(40 + P)
    ids, episode = np.arange(n), np.zeros(n, np.int64)
    ended = 0
    outs = [dict(done=Buf.full(kind, (n,), np.uint8, 7), lines=Buf.full(kind, (P, n), np.uint8, 7), dead=Buf.full(kind, (P, n), np.uint8, 7)) for _ in range(2)]
    for s in range(steps):
        player = rng.integers(0, P, n)
        mode = MODES[s % 2]
        cnt, lens, keys, pl = _device_lists(kind, a, player, False, L=L, K=K)
        cols = Buf.full(kind, (L, P, 10, n), np.uint32)
        a.simulate_lists_dev(cnt.ptr, lens.ptr, keys.ptr, cols.ptr, max_lists=L, max_keys=K, player=pl.ptr)
        phi = (rng.random((n, 20, 10, 7)) + 0.1).astype(F32)
        count = cnt.get()
        calls = [Call(kind, b, phi, player, count, cols, L, mode, seed=9, draw=s) for b in (a, c)]
        oa, oc = outs
        a.step_lists_eval_dev(calls[0].e, lens.ptr, keys.ptr, oa["done"].ptr, oa["lines"].ptr, oa["dead"].ptr, max_keys=K, auto_reset=auto)
        c.select_lists_dev(calls[1].e)
        c.step_lists_dev(calls[1].out["choice"].ptr, calls[1].cnt.ptr, lens.ptr, keys.ptr, oc["done"].ptr, oc["lines"].ptr, oc["dead"].ptr,
                         max_lists=L, max_keys=K, player=calls[1].pl.ptr, auto_reset=auto)
        ga, gc = calls[0].get(), calls[1].get()
        for name in ga:
            assert np.array_equal(ga[name].view(np.uint8), gc[name].view(np.uint8)), f"step {s}: '{name}'"
        for name in oa:
            assert np.array_equal(oa[name].get(), oc[name].get()), f"step {s}: '{name}'"
        assert np.array_equal(a.snapshot(), c.snapshot()), f"step {s}: the fused call against select + step_lists"
        assert (count >= 1).all() and (ga["choice"] >= 0).all() and (ga["choice"] < count).all()
        ln, kk = lens.get(), keys.get()                                      # the oracle steps the chosen key list
        keys_h, lens_h = np.zeros((n, P, K), np.uint8), np.ones((n, P), np.uint8)
        keys_h[ids, player] = kk[ids, ga["choice"]]
        lens_h[ids, player] = ln[ids, ga["choice"]]
        o.make_actions(keys_h, lens_h)
        done = o.finish_actions(400)
        rec = o.observe()[0]
        assert np.array_equal(oa["done"].get(), done), f"step {s}: done"
        assert np.array_equal(oa["lines"].get(), rec["reward"].T) and np.array_equal(oa["dead"].get(), rec["dead"].T), f"step {s}: lines / dead"
        finished = np.nonzero(done)[0].astype(np.int32)
        ended += len(finished)
        if auto and len(finished):
            episode[finished] += 1
            o.reset(finished, seeds=orc.episode_seed(ids[finished], episode[finished]))
        engines.assert_same_state(a, o, where=f"step {s}: against the oracle")
    assert a.take_errors() == 0 and c.take_errors() == 0
    if auto:
        assert ended > 0, "no game finished: auto-reset is not inside the comparison"


# ---------------------------------------------------------------- 6. arguments
def test_arguments_are_checked():
    pkg = ge.package()
    n, L, H = 4, 8, 20
    b, o = midgame("harness", n, 2, steps=3)
    phi, se = np.zeros((n, H, 10, 7), F32), np.zeros((n, 7), F32)
    cnt, cols, choice = np.zeros(n, np.int32), np.zeros((L, 2, 10, n), np.uint32), np.full(n, 9, np.int32)
    value, ent, plane = np.zeros((2, n), F32), np.zeros(n, F32), np.zeros((n, H, 10), F32)
    lens, keys = np.ones((n, L), np.uint8), np.zeros((n, L, 48), np.uint8)
    p = lambda arr: arr.ctypes.data                                                           # noqa: E731
    assert p(phi) % 16 == 0 and p(plane) % 16 == 0
    bad = [
        (dict(phi=None), "NULL"),
        (dict(count=None), "NULL"),
        (dict(cols=None), "NULL"),
        (dict(choice=None), "NULL"),
        (dict(n_pieces=5), "n_pieces"),
        (dict(n_pieces=0), "n_pieces"),
        (dict(state_eval=p(se), n_values=5), "n_values"),
        (dict(value=p(value)), "state_eval"),
        (dict(mode=2), "mode"),
        (dict(mode=3), "mode"),
        (dict(mode=-1), "mode"),
        (dict(mode="argmax", entropy=p(ent)), "entropy"),
        (dict(flags=8), "flag"),
        (dict(max_lists=0), "max_lists"),
        (dict(max_lists=257), "max_lists"),
        (dict(phi=p(phi) + 4), "aligned"),
        (dict(delta=p(plane) + 8), "aligned"),
        (dict(sums=p(plane) + 4), "aligned"),
    ]
    for kw, text in bad:
        args = dict(phi=p(phi), count=p(cnt), cols=p(cols), choice=p(choice), max_lists=L)
        args.update(kw)
        e = b.plan_eval(args.pop("phi"), args.pop("count"), args.pop("cols"), args.pop("choice"), **args)
        for call in (lambda: b.select_lists_dev(e), lambda: b.step_lists_eval_dev(e, p(lens), p(keys), None, None, None)):
            with pytest.raises(pkg.TetrisError, match=text):
                call()
    e = b.plan_eval(p(phi), p(cnt), p(cols), p(choice), max_lists=L)
    for call in (lambda: b.select_lists_dev(None), lambda: b.step_lists_eval_dev(None, p(lens), p(keys), None, None, None),
                 lambda: b.step_lists_eval_dev(e, None, p(keys), None, None, None), lambda: b.step_lists_eval_dev(e, p(lens), None, None, None, None)):
        with pytest.raises(pkg.TetrisError, match="NULL"):
            call()
    assert b.lib.tetris_step_lists_eval_dev(b._h, ctypes.byref(e), p(lens), p(keys), 48, 400, 2, None, None, None) == -1 and b"flag" in b.lib.tetris_last_error()
    s = pkg.TetrisBatch(n, 2, 20, 10, lib_path=ge.build_harness(), split_side=0)
    for call in (lambda: s.select_lists_dev(e), lambda: s.step_lists_eval_dev(e, p(lens), p(keys), None, None, None)):
        with pytest.raises(pkg.TetrisError, match="split"):
            call()
    assert np.all(choice == 9), "a rejected call must not run"
    engines.assert_same_state(b, o, where="a rejected call must not run")
    b.select_lists_dev(e)                                                   # the struct itself is good
    assert np.all(choice == 0) and pkg.capi.PLAN_OUT_F16 == 4


# ---------------------------------------------------------------- 7. torch interface (GPU only)
def _torch_phi(torch, phi):
    return torch.from_numpy(phi.view(np.int16) if phi.dtype == np.float16 else phi).cuda().view(torch.float16 if phi.dtype == np.float16 else torch.float32)


@pytest.mark.gpu
def test_torch_env_calls_equal_the_c_level_results():
    torch = pytest.importorskip("torch")
    ti = importlib.import_module("drl-tetris_amd.torch_interop")
    n, P, L, K = 64, 3, 64, 48
    rng = np.random.default_rng(70)
    a, c, o = midgame("hip", n, P, extra=1)
    te = ti.TorchEnv(a)
    player = rng.integers(0, P, n).astype(np.uint8)
    pt = torch.from_numpy(player).cuda()
    names = ("choice", "piece", "prob", "value", "entropy", "delta", "sums", "probs")
    for draw, (dtype, mode) in enumerate([(np.float32, "argmax"), (np.float32, "pi"), (np.float16, "pi"), (np.float16, "argmax")]):
        phi = crafted_phi(rng, n, 20, 7, dtype)
        se = rng.standard_normal((n, 8)).astype(dtype)
        cnt, lens, keys, pl = _device_lists("hip", c, player, False, L=L, K=K)
        cols = Buf.full("hip", (L, P, 10, n), np.uint32)
        c.simulate_lists_dev(cnt.ptr, lens.ptr, keys.ptr, cols.ptr, max_lists=L, max_keys=K, player=pl.ptr)
        out_f16 = dtype == np.float16
        call = Call("hip", c, phi, player, cnt.get(), cols, L, mode, state_eval=se, seed=21, draw=draw, out_f16=out_f16)
        c.select_lists_dev(call.e)
        want = call.get()
        te.action_lists(player=pt, max_lists=L, max_keys=K)
        got = te.choose_lists(_torch_phi(torch, phi), _torch_phi(torch, se), mode=mode, player=pt, seed=21, draw=draw,
                              out_dtype=torch.float16 if out_f16 else None, probs=True)
        torch.cuda.synchronize()
        assert np.array_equal(te.list_count.cpu().numpy(), cnt.get())
        for name, t in zip(names, got):
            if name == "entropy" and mode != "pi":
                assert t == 0.0
                continue
            g = t.cpu().numpy()
            g = g.view(np.uint16) if g.dtype == np.float16 else g
            w = want[name].view(np.uint16) if want[name].dtype == np.float16 else want[name]
            assert np.array_equal(g.view(np.uint8).reshape(-1), np.ascontiguousarray(w).view(np.uint8).reshape(-1)), f"TorchEnv.choose_lists {mode} {np.dtype(dtype).name}: '{name}'"
    # step_lists_eval against the C-level call on the copy
    done, lines, dead = Buf.full("hip", (n,), np.uint8), Buf.full("hip", (P, n), np.uint8), Buf.full("hip", (P, n), np.uint8)
    for draw in range(2):
        phi = crafted_phi(rng, n, 20, 7, np.float32)
        cnt, lens, keys, pl = _device_lists("hip", c, player, False, L=L, K=K)
        cols = Buf.full("hip", (L, P, 10, n), np.uint32)
        c.simulate_lists_dev(cnt.ptr, lens.ptr, keys.ptr, cols.ptr, max_lists=L, max_keys=K, player=pl.ptr)
        call = Call("hip", c, phi, player, cnt.get(), cols, L, "pi", seed=4, draw=draw)
        c.step_lists_eval_dev(call.e, lens.ptr, keys.ptr, done.ptr, lines.ptr, dead.ptr, max_keys=K, auto_reset=True)
        te.action_lists(player=pt, max_lists=L, max_keys=K)
        out = te.step_lists_eval(_torch_phi(torch, phi), mode="pi", player=pt, seed=4, draw=draw, auto_reset=True)
        torch.cuda.synchronize()
        want = call.get()
        assert np.array_equal(out[3].cpu().numpy(), want["choice"]) and np.array_equal(bits(out[5].cpu().numpy()), bits(want["prob"]))
        assert np.array_equal(out[0].cpu().numpy(), done.get()) and np.array_equal(out[1].cpu().numpy(), lines.get())
        assert np.array_equal(out[2].cpu().numpy(), dead.get()) and np.array_equal(out[4].cpu().numpy(), want["piece"]) and out[6] is None
        for name, t in (("entropy", out[7]), ("delta", out[8]), ("sums", out[9])):
            assert np.array_equal(bits(t.cpu().numpy()), bits(want[name])), f"TorchEnv.step_lists_eval: '{name}'"
        assert np.array_equal(a.snapshot(), c.snapshot()), "TorchEnv.step_lists_eval against the C-level call"
    assert a.take_errors() == 0 and c.take_errors() == 0
    a.set_stream(None, external=False)


@pytest.mark.gpu
def test_full_size_matches_the_torch_composition():
    """4 096 two-player games after 18 steps, 64 lists, strictly positive phi: the call against the composition it replaces —
    TorchEnv.deltas, the gather of the piece's plane, (deltas * phi_p).sum((1, 2)), the normalisation, argmax — on the device.
    probs within the relative tolerance 2 (H + L + 12) 2^-24 (both sides are float32 sums of positive terms with at most
    H + L + 12 roundings each); the choice in every game whose two highest q differ by more than that; those left out are at most
    1 % of the games.  (On the CPU harness the same 4 096 boards with numpy's random phi of three seeds leave out 9, 10 and 11
    games, 0.25 %, every one an exact tie: two key lists that end in the same afterstate.)"""
    torch = pytest.importorskip("torch")
    ti = importlib.import_module("drl-tetris_amd.torch_interop")
    n, L, H = 4096, 64, 20
    b = engines.make("hip", n, 2, seeds=orc.episode_seed(np.arange(n), 2))
    b.rollout_random(1, 18)
    te = ti.TorchEnv(b)
    pt = (torch.arange(n, device="cuda") % 2).to(torch.uint8)
    gen = torch.Generator(device="cuda").manual_seed(99)
    phi = torch.rand(n, H, 10, 7, generator=gen, device="cuda") + 0.1
    count, _, _ = te.action_lists(player=pt, max_lists=L)
    choice, piece, prob, _, _, delta, sums, probs = te.choose_lists(phi, mode="argmax", player=pt, probs=True)
    d, s = te.deltas(player=pt)
    phi_p = phi[torch.arange(n, device="cuda"), :, :, piece.long()]
    score = (d * phi_p.unsqueeze(-1)).sum(dim=(1, 2))
    want = score / score.sum(dim=1, keepdim=True)
    want_choice = want.argmax(dim=1)
    tol = 2 * (H + L + 12) * 2.0 ** -24
    top = want.double().topk(2, dim=1).values
    clear = (top[:, 0] - top[:, 1]) > tol * top[:, 0]
    rel = ((probs.double() - want.double()).abs() / torch.maximum(probs.double(), want.double()).clamp_min(1e-300)).max().item()
    left_out = int((~clear).sum().item())
    print(f"probs: largest relative difference {rel:.3g} (tolerance {tol:.3g}); {left_out} of {n} games are near-ties")
    assert (want > 0).any(dim=1).all() and rel <= tol
    assert left_out <= n // 100
    assert torch.equal(choice.long()[clear], want_choice[clear])
    assert torch.equal(delta, d[torch.arange(n, device="cuda"), :, :, choice.long()]) and torch.equal(sums, s[..., 0])
    assert torch.equal(prob, probs[torch.arange(n, device="cuda"), choice.long()])
    torch.cuda.synchronize()
    assert b.take_errors() == 0
    b.set_stream(None, external=False)

