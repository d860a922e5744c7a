"""Trajectory windows of a planning agent (include/tetris_hip.h: tetris_traj_record_plan_dev, tetris_traj_plan_batch_dev): the
packed record of a step's two [H][10] planes and its expansion into a minibatch.  The expansion of a recorded row is compared,
bit for bit, with the planes tetris_select_lists_dev writes for the same inputs (float32 and binary16, small_fill 1e-3 and 0);
the record's words with a numpy packer written here from the header's text; the batch semantics (permutations, entries that
name no sample, the mirror image, NULL outputs) with a numpy expansion written from the header's text; the whole path —
observe, record_plan, advantages, select, batch, plan_batch — with what the reference's sherlock_trajectory returned for seeded
episodes (tests/golden/traj_plan.npz, written by tests/golden/make_traj_plan_golden.py).  The tests parametrised over
engines.ENGINE_PARAMS run on the CPU harness (`-m "not gpu"`) and on the MI355X (`-m gpu`); on the harness the "device" buffers
are numpy arrays.  Every test closes the batches it opens."""
import importlib
import os

import numpy as np
import pytest

import __graft_entry__ as ge
from oracle import oracle as orc
from tests import engines, replay
from tests.act_support import midgame
from tests.buffers import GUARD, MIRROR, Buf, bits, out
from tests.plan_support import Call, _crafted, _device_lists, _words, crafted_phi

F32, U32, U8, I32 = np.float32, np.uint32, np.uint8, np.int32
GOLDEN = os.path.join(replay.GOLDEN, "traj_plan.npz")
WORDS = 112


# ---------------------------------------------------------------- buffers
class PlanWindow:
    """A window of T rows of the batch's games with its observation and plan records; every array has guard bytes behind it and
    starts as GUARD bytes throughout, so what a call did not write shows."""
    SHAPES = dict(action=(lambda T, n, S: (T, n, 4), U8), prob=(lambda T, n, S: (T, n), F32), value=(lambda T, n, S: (2, T, n), F32),
                  reward=(lambda T, n, S: (T, n), F32), done=(lambda T, n, S: (T, n), U8), obs=(lambda T, n, S: (T, n, S, 12), U32),
                  rec=(lambda T, n, S: (T, n, WORDS), U32))

    def __init__(self, kind, b, T):
        n, S = b.n_games, b.n_players
        self.kind, self.b, self.T, self.n, self.S = kind, b, T, n, S
        self.bufs = {k: out(kind, shape(T, n, S), dt) for k, (shape, dt) in self.SHAPES.items()}
        p = lambda k: self.bufs[k].ptr                                                           # noqa: E731
        self.traj = b.traj(T, p("action"), p("prob"), p("value"), p("reward"), p("done"))
        self.tobs = b.traj_obs(T, p("obs"))
        self.plan = b.traj_plan(T, p("rec"))

    def get(self, name):
        return self.bufs[name].get()

    def untouched(self, names=None, rows=None):
        for k in names or self.SHAPES:
            a = self.get(k)
            a = a if rows is None else (a[:, rows] if k == "value" else a[rows])
            if not (a.view(U8) == GUARD).all():
                return False
        return True


def run_plan_batch(kind, b, plan, index, fill, f16=False, delta=True, sums=True):
    """tetris_traj_plan_batch_dev of the index list -> {name: numpy [M, H, 10]} (guard bytes behind both outputs)"""
    M, H = len(index), b.height
    dt = np.float16 if f16 else F32
    ib = Buf(kind, np.asarray(index, np.int64).astype(U32).view(I32)) if M else None
    outs = {k: out(kind, (M, H, 10), dt) for k, on in (("delta", delta), ("sums", sums)) if on}
    b.traj_plan_batch_dev(plan, ib.ptr if M else 16, M, delta=outs["delta"].ptr if delta else None, sums=outs["sums"].ptr if sums else None,
                          small_fill=fill, f16=f16)
    return {k: v.get() for k, v in outs.items()}


def raw(a):
    """the bits of a float32 or float16 array"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint16) if a.dtype == np.float16 else a.view(U32)


# ---------------------------------------------------------------- the record and its expansion, from the header's text
def list_kinds(before, after, count):
    """before bool [N, H, 10], after bool [N, L, H, 10], count [N] -> (cnt [N], kind [N, L]: 0 NORMAL, 1 SMALL, 2 past count)"""
    L = after.shape[1]
    cnt = np.clip(count, 0, L)
    valid = np.arange(L)[None, :] < cnt[:, None]
    s = (after.astype(np.int32) - before[:, None].astype(np.int32)).sum(axis=(2, 3))
    return cnt, np.where(~valid, 2, np.where(s < 4, 1, 0))


def pack_records(before, after, count, choice):
    """-> uint32 [N, 112]: words 0..9 before, 10..19 the chosen list's columns (zero unless NORMAL), 20 its kind (2: no list), 21
    n_small | n_normal << 16, 22 + 9 c + j bit-plane j of column c's per-row counts over the NORMAL lists"""
    N, L, H = after.shape[:3]
    cnt, kind = list_kinds(before, after, count)
    ch = np.clip(choice, 0, np.maximum(cnt, 1) - 1)
    ck = np.where(cnt == 0, 2, kind[np.arange(N), ch])
    rec = np.zeros((N, WORDS), U32)
    rec[:, 0:10] = _words(before)
    rec[:, 10:20] = np.where((ck == 0)[:, None], _words(after[np.arange(N), ch]), 0)
    rec[:, 20] = ck
    rec[:, 21] = (kind == 1).sum(axis=1) | ((kind == 0).sum(axis=1) << 16)
    cells = (after & (kind == 0)[:, :, None, None]).sum(axis=1).astype(U32)                    # [N, H, 10] counts
    for c in range(10):
        for j in range(9):
            rec[:, 22 + 9 * c + j] = (((cells[:, :, c] >> j) & 1) << np.arange(H, dtype=U32)[None, :]).sum(axis=1)
    return rec, ck


def expand(rec, index, total, H, fill, f16):
    """rec uint32 [total, 112], index [M] -> (delta, sums) [M, H, 10], float32 or float16: the header's BATCH"""
    e = np.asarray(index, np.int64).astype(U32)
    at, mir = (e & U32(0x7FFFFFFF)).astype(np.int64), (e >> 31) == 1
    valid = at < total
    r = np.where(valid[:, None], rec[np.where(valid, at, 0)], 0).astype(U32)
    col = lambda w: np.where(mir[:, None], w[:, ::-1], w)                                       # noqa: E731
    y = np.arange(H, dtype=U32)[None, :, None]
    bit = lambda w: ((col(w)[:, None, :] >> y) & 1).astype(np.int32)                            # noqa: E731  -> [M, H, 10]
    b, a = bit(r[:, 0:10]), bit(r[:, 10:20])
    kind = r[:, 20][:, None, None]
    delta = np.where(kind == 0, (a - b).astype(F32), np.where(kind == 1, F32(fill), F32(0.0))).astype(F32)
    n_small, n_normal = (r[:, 21] & 0xFFFF).astype(np.int32), (r[:, 21] >> 16).astype(np.int32)
    planes = r[:, 22:].reshape(-1, 10, 9)
    cnt = sum(bit(planes[:, :, j]) << j for j in range(9))
    sums = (cnt - n_normal[:, None, None] * b).astype(F32) + (F32(fill) * n_small.astype(F32))[:, None, None]
    with np.errstate(over="ignore"):
        return (delta.astype(np.float16), sums.astype(F32).astype(np.float16)) if f16 else (delta, sums.astype(F32))


def reward_of(done, dead, who):
    """tetris_traj_record_dev's reward: done [N], dead [P, N], who [N]"""
    P, N = dead.shape
    me = dead[who, np.arange(N)] != 0
    you = dead[1 - who, np.arange(N)] != 0 if P > 1 else np.zeros(N, bool)
    return np.where(done != 0, np.where(me & you, -1.0, you.astype(F32) - me.astype(F32)), 0.0).astype(F32)


# ---------------------------------------------------------------- 1. record + expansion = the choosing call's planes
@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("P,H,L", [(1, 20, 7), (2, 20, 64), (2, 7, 1), (1, 31, 256), (2, 20, 130)])
def test_record_then_expand_equals_the_choose_calls_planes(kind, P, H, L):
    """67 crafted games (no multiple of either workgroup's 32), mixed and out-of-range players, counts from {-1, 0, .., L, L + 5}:
    rows 0 and 2 of a three-row window, argmax and pi, small_fill 1e-3 and 0."""
    N, T = 67, 3
    b, player, count, cols, before, after = _crafted(kind, N, P, H, L, seed=100 * P + H + L)
    try:
        who = np.minimum(player, P - 1)
        rng = np.random.default_rng(11 * P + H + L)
        w = PlanWindow(kind, b, T)
        pl = Buf.full(kind, (N,), U8)
        pl.put(player)
        blob = b.snapshot()
        for row, mode, fill in ((0, "argmax", 1e-3), (2, "pi", 0.0), (2, "argmax", 0.0), (0, "pi", 1e-3)):
            where = f"row {row} {mode} fill {fill}"
            phi = crafted_phi(rng, N, H, 7, F32)
            se = rng.standard_normal((N, 7)).astype(F32)
            done = (rng.random(N) < 0.5).astype(U8)
            dead = (rng.random((P, N)) < 0.5).astype(U8)
            db, xb = Buf(kind, done), Buf(kind, dead)
            b.traj_observe_dev(w.tobs, row, pl.ptr)
            call = Call(kind, b, phi, player, count, cols, L, mode, fill=fill, state_eval=se, seed=31, draw=row)
            half = Call(kind, b, phi, player, count, cols, L, mode, fill=fill, seed=31, draw=row, out_f16=True)
            b.select_lists_dev(call.e)
            b.select_lists_dev(half.e)
            want, wanth = call.get(), half.get()
            assert np.array_equal(want["choice"], wanth["choice"])
            b.traj_record_plan_dev(w.traj, w.plan, w.tobs, row, call.e, db.ptr, xb.ptr)
            index = row * N + np.arange(N)
            got = run_plan_batch(kind, b, w.plan, index, fill)
            goth = run_plan_batch(kind, b, w.plan, index, fill, f16=True)
            for name in ("delta", "sums"):
                assert np.array_equal(raw(got[name]), raw(want[name])), f"{where}: float32 '{name}' differs in games {np.unique(np.argwhere(raw(got[name]) != raw(want[name]))[:, 0])[:8]}"
                assert np.array_equal(raw(goth[name]), raw(wanth[name])), f"{where}: binary16 '{name}' differs"
            # the row arrays
            cnt = np.clip(count, 0, L)
            assert np.array_equal(w.get("action")[row], np.stack([want["choice"] & 255, np.zeros(N, I32), want["piece"], who], axis=1)), f"{where}: 'action'"
            assert np.array_equal(bits(w.get("prob")[row]), bits(want["prob"])), f"{where}: 'prob'"
            assert np.array_equal(bits(w.get("value")[:, row]), bits(want["value"])), f"{where}: 'value'"
            assert np.array_equal(w.get("done")[row], done), f"{where}: 'done'"
            assert np.array_equal(w.get("reward")[row], reward_of(done, dead, who)), f"{where}: 'reward'"
            # the record is the documented one
            rec, ck = pack_records(before, after, count, want["choice"])
            assert np.array_equal(w.get("rec")[row], rec), f"{where}: the record differs in games {np.unique(np.argwhere(w.get('rec')[row] != rec)[:, 0])[:8]}"
            assert (cnt == 0).any() and (ck == 2).sum() == (cnt == 0).sum()
        assert w.untouched(("action", "prob", "value", "reward", "done", "obs", "rec"), rows=1), "only the rows asked for are written"
        assert np.array_equal(b.snapshot(), blob), "the batch's state was written"
        assert b.take_errors() == 0
    finally:
        b.close()


# ---------------------------------------------------------------- 2. the record's words
@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
def test_the_records_words_are_the_documented_format(kind):
    """35 one-player games on empty boards with 256, 255 or 254 lists the test fills cell by cell, every one NORMAL: four cells
    that all of a game's lists fill — with 256 lists plane 8 is set there and planes 0..7 are clear — and one more cell that goes
    round with the list number.  Game 1 has count 0 (kind 2), game 2's list 5 is SMALL and chosen, game 3 holds SMALL lists that
    are not chosen; the choices run past both ends of [0, count) and are clamped."""
    N, L, H, T = 35, 256, 20, 2
    b = engines.make(kind, N, 1, height=H, seeds=orc.episode_seed(np.arange(N), 1))
    try:
        before = b.observe()[0]["field"][:, 0, :H] > 0
        assert not before.any()
        after = np.zeros((N, L, H, 10), bool)
        rng = np.random.default_rng(256)
        count = (L - np.arange(N) % 3).astype(I32)
        count[1] = 0
        full = np.zeros((N, 4), np.int64)
        for i in range(N):
            cells = rng.permutation(H * 10)[:11]
            full[i] = cells[:4]
            for k in range(L):
                after[i, k].reshape(-1)[cells[:4]] = True
                after[i, k].reshape(-1)[cells[4 + k % 7]] = True
        after[2, 5] = False
        after[2, 5].reshape(-1)[:2] = True
        after[3, 7:11] = False
        choice = rng.integers(-3, L + 8, N).astype(I32)
        choice[2], choice[0], choice[6] = 5, L + 40, -9
        cols = np.ascontiguousarray(_words(after).transpose(1, 2, 0)[:, None])                  # [L, 1, 10, N]
        w = PlanWindow(kind, b, T)
        bufs = dict(count=Buf(kind, count), cols=Buf(kind, cols), choice=Buf(kind, choice), piece=Buf(kind, (np.arange(N) % 7).astype(U8)),
                    prob=Buf(kind, rng.random(N).astype(F32)), done=Buf(kind, np.zeros(N, U8)), dead=Buf(kind, np.zeros((1, N), U8)))
        e = b.plan_eval(None, bufs["count"].ptr, bufs["cols"].ptr, bufs["choice"].ptr, max_lists=L, piece=bufs["piece"].ptr, prob=bufs["prob"].ptr)
        b.traj_observe_dev(w.tobs, 1, None)
        b.traj_record_plan_dev(w.traj, w.plan, w.tobs, 1, e, bufs["done"].ptr, bufs["dead"].ptr)
        got = w.get("rec")[1]
        want, ck = pack_records(before, after, count, choice)
        assert np.array_equal(got, want), f"the record differs in games {np.unique(np.argwhere(got != want)[:, 0])[:8]}"
        assert ck[1] == 2 and ck[2] == 1 and got[2, 20] == 1 and not got[2, 10:20].any() and got[1, 20] == 2 and got[1, 21] == 0
        assert got[2, 21] == 1 | (253 << 16) and got[3, 21] == 4 | (252 << 16) and got[0, 21] == 256 << 16
        for i in np.nonzero(count == 256)[0]:
            if i in (2, 3):
                continue
            for cell in full[i]:
                y, c = divmod(int(cell), 10)
                planes = (got[i, 22 + 9 * c: 31 + 9 * c] >> y) & 1
                assert planes.tolist() == [0] * 8 + [1], f"game {i}: a cell that 256 lists fill"
        clamped = np.clip(choice, 0, np.maximum(np.clip(count, 0, L), 1) - 1)
        assert np.array_equal(w.get("action")[1], np.stack([clamped & 255, np.zeros(N, I32), np.arange(N) % 7, np.zeros(N, I32)], axis=1))
        assert np.array_equal(w.get("value")[:, 1], np.zeros((2, N), F32)), "no d_value: zeros"
        # the sums of the expansion there are the list count, 256 included
        sums = run_plan_batch(kind, b, w.plan, N + np.arange(N), 1e-3, delta=False)["sums"]
        assert sums[0].reshape(-1)[full[0]].tolist() == [256.0] * 4
        assert w.untouched(rows=0)
        assert b.take_errors() == 0
    finally:
        b.close()


# ---------------------------------------------------------------- 3. after a real step
@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("auto", [False, True], ids=["plain", "auto_reset"])
@pytest.mark.parametrize("P", [1, 2])
def test_a_recorded_step_expands_to_the_planes_taken_before_it(kind, P, auto):
    """64 mid-game games, six decisions into a three-row window: action_lists, simulate, observe(row), select_lists (its planes
    copied), step_lists_eval with the same struct (the same choice), record_plan(row) — after the step, from boards that have
    moved on.  The expansion of the row equals the copied planes and the games equal the oracle's."""
    n, L, K, T, steps = 64, 64, 48, 3, 6
    a, o = midgame(kind, n, P)
    try:
        rng = np.random.default_rng(50 + P)
        ids, episode, ended = np.arange(n), np.zeros(n, np.int64), 0
        w = PlanWindow(kind, a, T)
        done, lines, dead = Buf.full(kind, (n,), U8, 7), Buf.full(kind, (P, n), U8, 7), Buf.full(kind, (P, n), U8, 7)
        for s in range(steps):
            row, mode, fill = s % T, ("argmax", "pi")[s % 2], (1e-3, 0.0)[(s // 2) % 2]
            player = rng.integers(0, P, n)
            cnt, lens, keys, pl = _device_lists(kind, a, player, False, L=L, K=K)
            cols = Buf.full(kind, (L, P, 10, n), U32)
            a.simulate_lists_dev(cnt.ptr, lens.ptr, keys.ptr, cols.ptr, max_lists=L, max_keys=K, player=pl.ptr)
            a.traj_observe_dev(w.tobs, row, pl.ptr)
            phi = (rng.random((n, 20, 10, 7)) + 0.1).astype(F32)
            call = Call(kind, a, phi, player, cnt.get(), cols, L, mode, fill=fill, seed=9, draw=s)
            a.select_lists_dev(call.e)
            kept = call.get()
            a.step_lists_eval_dev(call.e, lens.ptr, keys.ptr, done.ptr, lines.ptr, dead.ptr, max_keys=K, auto_reset=auto)
            assert np.array_equal(call.get()["choice"], kept["choice"])
            a.traj_record_plan_dev(w.traj, w.plan, w.tobs, row, call.e, done.ptr, dead.ptr)
            got = run_plan_batch(kind, a, w.plan, row * n + np.arange(n), fill)
            assert np.array_equal(raw(got["delta"]), raw(kept["delta"])) and np.array_equal(raw(got["sums"]), raw(kept["sums"])), f"step {s}"
            assert (kept["delta"] != 0).any() and np.array_equal(w.get("action")[row][:, 0], kept["choice"] & 255)
            assert np.array_equal(w.get("reward")[row], reward_of(done.get(), dead.get(), player)), f"step {s}: reward"
            ln, kk = lens.get(), keys.get()                                      # the oracle steps the chosen key list
            keys_h, lens_h = np.zeros((n, P, K), U8), np.ones((n, P), U8)
            keys_h[ids, player] = kk[ids, kept["choice"]]
            lens_h[ids, player] = ln[ids, kept["choice"]]
            o.make_actions(keys_h, lens_h)
            d = o.finish_actions(400)
            assert np.array_equal(done.get(), d), f"step {s}: done"
            finished = np.nonzero(d)[0].astype(I32)
            ended += len(finished)
            if auto and len(finished):
                episode[finished] += 1
                o.reset(finished, seeds=orc.episode_seed(ids[finished], episode[finished]))
            engines.assert_same_state(a, o, where=f"step {s}: against the oracle")
        assert a.take_errors() == 0
    finally:
        a.close()


# ---------------------------------------------------------------- 4. batch semantics
@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("H,f16", [(20, False), (20, True), (7, True), (31, True), (7, False)])
def test_batch_semantics(kind, H, f16):
    """Records of random words (kinds 0, 1, 2) in a window of 3 x 67 entries; M = 0, 1, 65 and 1 000: a permutation with repeats,
    -1, T N and T N + 5 (zeros), entries with bit 31 (the unmirrored expansion with the column axis reversed), either output NULL.
    Heights 7 and 31 in binary16 are the odd run lengths: a sample is 140 or 620 bytes."""
    T, N = 3, 67
    total = T * N
    rng = np.random.default_rng(H + 2 * f16)
    b = engines.make(kind, N, 1, height=H)
    try:
        rec = rng.integers(0, 1 << 32, (total, WORDS), dtype=np.uint64).astype(U32)
        rec[:, 20] = rng.integers(0, 3, total)
        rec[:, 21] = rng.integers(0, 300, total) | (rng.integers(0, 300, total) << 16)
        rb = Buf(kind, rec)
        plan = b.traj_plan(T, rb.ptr)
        fill = 1e-3
        for M in (0, 1, 65, 1000):
            index = rng.integers(0, total, M).astype(np.int64)
            if M >= 65:
                index[3], index[17], index[40], index[M - 1] = -1, total, total + 5, total - 1
                index[5] = (total + 5) | MIRROR
            mirrored = rng.random(M) < 0.5
            if M == 1:
                mirrored[:] = True
            index = np.where(mirrored & (index >= 0), index | MIRROR, index)
            got = run_plan_batch(kind, b, plan, index, fill, f16=f16)
            want = dict(zip(("delta", "sums"), expand(rec, index, total, H, fill, f16)))
            for name in ("delta", "sums"):
                assert got[name].shape == (M, H, 10) and np.array_equal(raw(got[name]), raw(want[name])), f"M={M}: '{name}' differs from the header's text"
            if M == 0:
                continue
            plain = run_plan_batch(kind, b, plan, np.where(index >= 0, index & ~MIRROR, index), fill, f16=f16)
            named = ((index & 0x7FFFFFFF) < total) & (index >= -MIRROR)
            for name in ("delta", "sums"):
                flipped = np.where((mirrored & named)[:, None, None], plain[name][:, :, ::-1], plain[name])
                assert np.array_equal(raw(got[name]), raw(flipped)), f"M={M}: '{name}' of a mirrored entry"
                assert not raw(got[name])[~named].any(), f"M={M}: an entry that names no sample"
            if M >= 65:
                assert (~named).sum() >= 4
                only_d = run_plan_batch(kind, b, plan, index, fill, f16=f16, sums=False)
                only_s = run_plan_batch(kind, b, plan, index, fill, f16=f16, delta=False)
                assert list(only_d) == ["delta"] and np.array_equal(raw(only_d["delta"]), raw(got["delta"]))
                assert list(only_s) == ["sums"] and np.array_equal(raw(only_s["sums"]), raw(got["sums"]))
        assert np.array_equal(rb.get(), rec)
        assert b.take_errors() == 0
    finally:
        b.close()


# ---------------------------------------------------------------- 5. the reference's numbers
@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
def test_the_fixture_through_the_whole_path(kind):
    """Every episode of tests/golden/traj_plan.npz is one game column of a window, at the window's end, with another finished
    episode in front of it.  Per row: the acting player's boards are restored to the fixture's `before`, observe, d_cols from its
    `after` fields, the choosing call's output arrays filled with its a_idx / piece / prob / values, then record_plan; then, per
    (gamma, gae_lambda) case, advantages, select, batch and plan_batch(small_fill = 0).  Compared per episode with the seven
    arrays the reference returned, in its order, and its r and d: integers and planes exactly, prob bit for bit after the float32
    cast, adv / target within 4e-6 absolute — the bound tests/test_traj_device.py establishes between this recurrence in float32
    and the reference's float64 (eight times the worst difference measured for the definition on values drawn from 2 N(0, 1)).
    Measured here: 2.45e-7 (adv) and 1.32e-7 (target)."""
    z = np.load(GOLDEN)
    E, H, L, P = len(z["case"]), 20, z["after"].shape[1], 2
    T = int(z["length"].max()) + 2
    b = engines.make(kind, E, P, height=H, seeds=orc.episode_seed(np.arange(E), 4))
    try:
        blob = b.snapshot()
        first_word = b.snapshot_words - P * b.lib.tetris_layout_words()                         # the acting player 0's column words
        rng = np.random.default_rng(5)
        w = PlanWindow(kind, b, T)
        span = [(int(z["start"][e]), int(z["length"][e]), T - int(z["length"][e])) for e in range(E)]
        for t in range(T):
            before, after = np.zeros((E, H, 10), bool), np.zeros((E, L, H, 10), bool)
            choice, piece = rng.integers(0, L, E).astype(I32), rng.integers(0, 7, E).astype(U8)
            prob, value = rng.random(E).astype(F32), (2.0 * rng.standard_normal((2, E))).astype(F32)
            done, dead = np.zeros(E, U8), np.zeros((P, E), U8)
            for e, (s, length, first) in enumerate(span):
                if t == first - 1:
                    done[e], dead[0, e] = 1, 1                                                  # the episode in front ends here
                if t >= first:
                    k = s + t - first
                    before[e], after[e], choice[e], piece[e], prob[e] = z["before"][k], z["after"][k], z["a_idx"][k], z["piece"][k], z["prob"][k]
                    value[0, e], value[1, e], done[e] = z["v_piece"][k], z["v_mean"][k], z["done"][k]
                    dead[0, e], dead[1, e] = z["reward"][k] < 0, z["reward"][k] > 0
            blob[:, first_word:first_word + 10] = _words(before)
            b.restore(blob)
            assert np.array_equal(b.observe()[0]["field"][:, 0, :H] > 0, before)
            cols = np.zeros((L, P, 10, E), U32)
            cols[:, 0] = _words(after).transpose(1, 2, 0)
            bufs = [Buf(kind, x) for x in (np.full(E, L, I32), cols, choice, piece, prob, value, done, dead)]
            e_ = b.plan_eval(None, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, max_lists=L, piece=bufs[3].ptr, prob=bufs[4].ptr, value=bufs[5].ptr)
            b.traj_observe_dev(w.tobs, t, None)
            b.traj_record_plan_dev(w.traj, w.plan, w.tobs, t, e_, bufs[6].ptr, bufs[7].ptr)
        adv, target, closed = (Buf(kind, np.zeros((T, E), dt)) for dt in (F32, F32, U8))
        index, count = Buf(kind, np.zeros(T * E, I32)), Buf(kind, np.zeros(1, I32))
        compared, worst = 0, [0.0, 0.0]
        for case in range(len(z["gamma"])):
            b.traj_advantages_dev(w.traj, T, float(z["gamma"][case]), float(z["gae_lambda"][case]), float(z["gve_lambda"]), None, adv.ptr, target.ptr, closed.ptr)
            b.traj_select_dev(closed.ptr, T, index.ptr, T * E, count.ptr)
            M = int(count.get()[0])
            idx = index.get()[:M]
            assert M == T * E and (idx >= 0).all(), "every column ends in a done: every entry is closed"
            outs = dict(visual=Buf(kind, np.zeros((P, M, H, 10), U8)), action=Buf(kind, np.zeros((M, 3), U8)), prob=Buf(kind, np.zeros(M, F32)),
                        adv=Buf(kind, np.zeros(M, F32)), target=Buf(kind, np.zeros(M, F32)), reward=Buf(kind, np.zeros(M, F32)),
                        done=Buf(kind, np.zeros(M, U8)))
            ib = Buf(kind, idx)
            b.traj_batch_dev(w.traj, w.tobs, ib.ptr, M, b.traj_batch(**{k: v.ptr for k, v in outs.items()}), adv=adv.ptr, target=target.ptr)
            mb = {k: v.get() for k, v in outs.items()}
            pl = run_plan_batch(kind, b, w.plan, idx, 0.0)
            for e in np.nonzero(z["case"] == case)[0]:
                s, length, first = span[e]
                j = np.nonzero((idx % E == e) & (idx // E >= first))[0]                           # ascending: in time order
                assert len(j) == length
                ref = [z[f"out{q}"][s:s + length] for q in range(7)]
                assert np.array_equal(mb["action"][j, 0], ref[0][:, 0]) and np.array_equal(mb["action"][j, 2], ref[1][:, 0]), f"episode {e}: a_idx / piece"
                assert np.array_equal(bits(mb["prob"][j]), bits(ref[2][:, 0].astype(F32))), f"episode {e}: prob"
                for q, name in ((3, "adv"), (4, "target")):
                    err = np.abs(mb[name][j].astype(np.float64) - ref[q][:, 0])
                    worst[q - 3] = max(worst[q - 3], float(err.max()))
                assert np.array_equal(pl["delta"][j].astype(np.float64), ref[5][..., 0]), f"episode {e}: delta"
                assert np.array_equal(pl["sums"][j].astype(np.float64), ref[6][..., 0]), f"episode {e}: delta_sum"
                assert np.array_equal(mb["reward"][j].astype(np.float64), z["r"][s:s + length, 0]) and np.array_equal(mb["done"][j], z["d"][s:s + length, 0])
                assert np.array_equal(mb["visual"][0][j] > 0, z["before"][s:s + length]), f"episode {e}: the states"
                compared += length
        print(f"largest difference from the reference: adv {worst[0]:.3g}, target {worst[1]:.3g} over {compared} entries")
        assert compared == len(z["a_idx"]) == 2 * (1 + 2 + 3 + 17), "every entry of the fixture is compared"
        assert (z["out5"] < 0).any() and (z["out5"] > 0).any() and (np.abs(z["out5"]).sum(axis=(1, 2, 3)) == 0).any(), "normal and small chosen lists"
        assert worst[0] <= 4e-6 and worst[1] <= 4e-6
        assert b.take_errors() == 0
    finally:
        b.close()


# ---------------------------------------------------------------- 6. arguments (harness only)
def test_arguments_are_checked():
    pkg = ge.package()
    n, T, L, H = 4, 3, 8, 20
    b, o = midgame("harness", n, 2, steps=3)
    others = []
    try:
        w = PlanWindow("harness", b, T)
        p = lambda arr: arr.ctypes.data                                                           # noqa: E731
        cnt, cols, choice = np.full(n, 2, I32), np.zeros((L, 2, 10, n), U32), np.full(n, 1, I32)
        piece, prob, value = np.zeros(n, U8), np.zeros(n, F32), np.zeros((2, n), F32)
        done, dead = np.zeros(n, U8), np.zeros((2, n), U8)
        ev = dict(count=p(cnt), cols=p(cols), choice=p(choice), max_lists=L, piece=p(piece), prob=p(prob), value=p(value))

        def struct(**kw):
            args = dict(ev, **kw)
            return b.plan_eval(None, args.pop("count"), args.pop("cols"), args.pop("choice"), **args)

        e = struct()
        record = lambda bb=b, traj=w.traj, plan=w.plan, obs=w.tobs, row=0, e=e, done=p(done), dead=p(dead): bb.traj_record_plan_dev(traj, plan, obs, row, e, done, dead)    # noqa: E731
        arrays = {k: w.bufs[k].ptr for k in ("action", "prob", "value", "reward", "done")}
        bad = [(dict(row=r), "row") for r in (-1, T, T + 100)]
        bad += [(dict(traj=b.traj(T, **dict(arrays, **{k: None}))), "NULL") for k in arrays]
        bad += [(dict(traj=b.traj(T + 1, **arrays)), "capacity"), (dict(plan=b.traj_plan(T - 1, w.bufs["rec"].ptr)), "capacity"),
                (dict(obs=b.traj_obs(T + 2, w.bufs["obs"].ptr)), "capacity")]
        bad += [(dict(e=None), "NULL"), (dict(traj=None), "NULL"), (dict(done=None), "NULL"), (dict(dead=None), "NULL"), (dict(obs=None), "NULL")]
        bad += [(dict(e=struct(**{k: None})), "NULL") for k in ("choice", "piece", "prob", "count", "cols")]
        bad += [(dict(obs=b.traj_obs(T, None)), "NULL"), (dict(plan=b.traj_plan(T, None)), "NULL")]
        bad += [(dict(e=struct(max_lists=0)), "max_lists"), (dict(e=struct(max_lists=257)), "max_lists")]
        bad += [(dict(plan=b.traj_plan(T, w.bufs["rec"].ptr + 4)), "aligned"), (dict(obs=b.traj_obs(T, w.bufs["obs"].ptr + 8)), "aligned")]
        for players in (3, 4):
            others.append(engines.make("harness", n, players))
            bad.append((dict(bb=others[-1], dead=p(np.zeros((players, n), U8))), "one or two players"))
        others.append(pkg.TetrisBatch(n, 2, 20, 10, lib_path=ge.build_harness(), split_side=0))
        bad.append((dict(bb=others[-1]), "split"))
        for kw, text in bad:
            with pytest.raises(pkg.TetrisError, match=text):
                record(**kw)
        assert w.untouched(), "a refused call writes nothing"
        # the batch call
        rec = np.zeros((T * n, WORDS), U32)
        index, planes = np.zeros(8, I32), np.full((2, 8, H, 10), -7.0, F32)
        assert p(rec) % 16 == 0 and p(planes) % 16 == 0
        batch = lambda bb=b, plan=b.traj_plan(T, p(rec)), index=p(index), M=8, flags=0, delta=p(planes[0]), sums=p(planes[1]): bb.traj_plan_batch_dev(plan, index, M, delta=delta, sums=sums, flags=flags)    # noqa: E731
        bad = [(dict(plan=None), "NULL"), (dict(plan=b.traj_plan(T, None)), "NULL"), (dict(index=None), "NULL"), (dict(delta=None, sums=None), "NULL"),
               (dict(M=-1), "M < 0"), (dict(plan=b.traj_plan(1 << 29, p(rec))), "2\\^31"), (dict(flags=2), "flag"), (dict(flags=1 << 31 >> 1), "flag"),
               (dict(plan=b.traj_plan(T, p(rec) + 4)), "aligned"), (dict(delta=p(planes[0]) + 8), "aligned"), (dict(sums=p(planes[1]) + 4), "aligned"),
               (dict(bb=others[0]), "one or two players"), (dict(bb=others[1]), "one or two players"), (dict(bb=others[2]), "split")]
        for kw, text in bad:
            with pytest.raises(pkg.TetrisError, match=text):
                batch(**kw)
        assert np.all(planes == F32(-7.0)), "a refused call writes nothing"
        engines.assert_same_state(b, o, where="a refused call must not run")
        # what is accepted: M = 0 with nothing else to go by, the structs that were refused piecewise, a plan-less record
        b.traj_plan_batch_dev(b.traj_plan(T, p(rec)), p(index), 0, delta=p(planes[0]))
        assert np.all(planes == F32(-7.0))
        batch()
        assert np.all(planes == F32(0.0))
        b.traj_record_plan_dev(w.traj, None, None, 1, struct(count=None, cols=None, max_lists=0, value=None), p(done), p(dead))
        assert w.untouched(("rec", "obs")) and w.untouched(rows=0) and w.untouched(rows=2), "plan = NULL: the row arrays only"
        assert np.array_equal(w.get("action")[1], np.stack([choice, 0 * choice, piece, 0 * choice], axis=1)) and not w.get("value")[:, 1].any()
        b.traj_observe_dev(w.tobs, 0, None)
        record()
        assert not w.untouched(("rec",), rows=0) and w.untouched(rows=2)
        engines.assert_same_state(b, o, where="the calls do not write the games")
        assert pkg.capi.PLAN_REC_WORDS == 112 and pkg.capi.PLAN_BATCH_F16 == 1
    finally:
        for x in [b] + others:
            x.close()


# ---------------------------------------------------------------- 7. torch interface (GPU only)
@pytest.mark.gpu
def test_torch_env_calls_equal_the_c_level_results():
    """Trajectory(plan=True).record_plan / batch_plan against the C-level calls on a copy of the games; planes=False returns None
    for the planes and the same choice."""
    torch = pytest.importorskip("torch")
    ti = importlib.import_module("drl-tetris_amd.torch_interop")
    n, P, L, K, T = 64, 2, 64, 48, 3
    rng = np.random.default_rng(71)
    a, c, o = midgame("hip", n, P, extra=1)
    try:
        te = ti.TorchEnv(a)
        tr = te.trajectory(T, states=True, plan=True)
        assert tuple(tr.plan_rec.shape) == (T, n, WORDS) and tr.plan_rec.dtype == torch.int32
        with pytest.raises(AssertionError):
            te.trajectory(T, plan=True)
        w = PlanWindow("hip", c, T)
        done, lines, dead = Buf.full("hip", (n,), U8), Buf.full("hip", (P, n), U8), Buf.full("hip", (P, n), U8)
        for s in range(4):
            row, mode = s % T, ("pi", "argmax")[s % 2]
            player = rng.integers(0, P, n).astype(U8)
            pt = torch.from_numpy(player).cuda()
            phi = crafted_phi(rng, n, 20, 7, F32)
            se = rng.standard_normal((n, 7)).astype(F32)
            cnt, lens, keys, pl = _device_lists("hip", c, player, False, L=L, K=K)
            cols = Buf.full("hip", (L, P, 10, n), U32)
            c.simulate_lists_dev(cnt.ptr, lens.ptr, keys.ptr, cols.ptr, max_lists=L, max_keys=K, player=pl.ptr)
            c.traj_observe_dev(w.tobs, row, pl.ptr)
            call = Call("hip", c, phi, player, cnt.get(), cols, L, mode, state_eval=se, seed=4, draw=s)
            c.step_lists_eval_dev(call.e, lens.ptr, keys.ptr, done.ptr, lines.ptr, dead.ptr, max_keys=K, auto_reset=True)
            c.traj_record_plan_dev(w.traj, w.plan, w.tobs, row, call.e, done.ptr, dead.ptr)
            want = call.get()
            te.action_lists(player=pt, max_lists=L, max_keys=K)
            tr.observe(row, pt)
            out = te.step_lists_eval(torch.from_numpy(phi).cuda(), torch.from_numpy(se).cuda(), mode=mode, player=pt, seed=4, draw=s,
                                     auto_reset=True, planes=s % 2 == 0)
            tr.record_plan(row)
            torch.cuda.synchronize()
            assert np.array_equal(out[3].cpu().numpy(), want["choice"]) and np.array_equal(bits(out[5].cpu().numpy()), bits(want["prob"]))
            if s % 2 == 0:
                assert np.array_equal(bits(out[8].cpu().numpy()), bits(want["delta"])) and np.array_equal(bits(out[9].cpu().numpy()), bits(want["sums"]))
            else:
                assert out[8] is None and out[9] is None
            assert np.array_equal(a.snapshot(), c.snapshot())
        for name, t in (("action", tr.action), ("prob", tr.prob), ("value", tr.value), ("reward", tr.reward), ("done", tr.done), ("obs", tr.obs),
                        ("rec", tr.plan_rec)):
            assert np.array_equal(t.cpu().numpy().view(U8), w.get(name).view(U8)), f"Trajectory: '{name}' differs from the C-level window"
        index = rng.integers(0, T * n, 200).astype(np.int64)
        index[::3] |= MIRROR
        index[7] = -1
        it = torch.from_numpy(index.astype(U32).view(I32)).cuda()
        for dtype, f16, fill in ((None, False, 1e-3), (torch.float16, True, 0.0)):
            got = tr.batch_plan(it, small_fill=fill, dtype=dtype)
            torch.cuda.synchronize()
            want = run_plan_batch("hip", c, w.plan, index, fill, f16=f16)
            assert tuple(got.delta.shape) == tuple(got.sums.shape) == (200, 20, 10, 1)
            for name in ("delta", "sums"):
                g = getattr(got, name).cpu().numpy()[..., 0]
                assert np.array_equal(raw(g), raw(want[name])), f"Trajectory.batch_plan: '{name}'"
        assert tr.batch_plan(it, small_fill=0.0, dtype=torch.float16) is got, "reused per (M, dtype)"
        te.action_lists(player=pt, max_lists=L, max_keys=K)
        full = [t.clone() for t in te.choose_lists(torch.from_numpy(phi).cuda(), mode="pi", player=pt, seed=8, draw=9)[:3]]
        lean = te.choose_lists(torch.from_numpy(phi).cuda(), mode="pi", player=pt, seed=8, draw=9, planes=False)
        torch.cuda.synchronize()
        assert lean[5] is None and lean[6] is None and all(torch.equal(x, y) for x, y in zip(full, lean[:3]))
        assert a.take_errors() == 0 and c.take_errors() == 0
        a.set_stream(None, external=False)
    finally:
        for x in (a, c):
            x.close()


@pytest.mark.gpu
def test_full_size_matches_the_torch_composition():
    """4 096 two-player games after 18 steps, 64 lists, a window of four rows: every row's float planes are kept from choose_lists
    in [T, n, H, 10] tensors, the way a user of the parent commit has to; a minibatch of 4 096 entries, half of them mirrored,
    against index_select and flip on those tensors: equal bits."""
    torch = pytest.importorskip("torch")
    ti = importlib.import_module("drl-tetris_amd.torch_interop")
    n, L, H, T, M = 4096, 64, 20, 4, 4096
    b = engines.make("hip", n, 2, seeds=orc.episode_seed(np.arange(n), 2))
    try:
        b.rollout_random(1, 18)
        te = ti.TorchEnv(b)
        tr = te.trajectory(T, states=True, plan=True)
        gen = torch.Generator(device="cuda").manual_seed(98)
        keep_d, keep_s = torch.zeros(T, n, H, 10, device="cuda"), torch.zeros(T, n, H, 10, device="cuda")
        for t in range(T):
            pt = ((torch.arange(n, device="cuda") + t) % 2).to(torch.uint8)
            phi = torch.rand(n, H, 10, 7, generator=gen, device="cuda") + 0.1
            te.action_lists(player=pt, max_lists=L)
            tr.observe(t, pt)
            out = te.step_lists_eval(phi, mode="pi", player=pt, seed=3, draw=t, auto_reset=True)
            keep_d[t].copy_(out[8])
            keep_s[t].copy_(out[9])
            tr.record_plan(t)
        index = torch.randint(0, T * n, (M,), generator=gen, device="cuda", dtype=torch.int64)
        mirrored = torch.arange(M, device="cuda") % 2 == 1
        packed = torch.where(mirrored, index | MIRROR, index).to(torch.int32)                     # (bit 31 wraps into the sign)
        got = tr.batch_plan(packed)
        for name, keep in (("delta", keep_d), ("sums", keep_s)):
            plain = keep.view(T * n, H, 10).index_select(0, index)
            want = torch.where(mirrored[:, None, None], plain.flip(2), plain)
            assert torch.equal(getattr(got, name)[..., 0].view(torch.int32), want.view(torch.int32)), f"'{name}' differs from index_select + flip"
        assert (keep_d != 0).any() and (keep_s > 1).any()
        torch.cuda.synchronize()
        assert b.take_errors() == 0
        b.set_stream(None, external=False)
    finally:
        b.close()
