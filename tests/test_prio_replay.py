"""The prioritised experience replay on the device (include/tetris_hip.h: tetris_replay_add_dev, tetris_replay_sample_dev,
tetris_replay_update_prios_dev, tetris_replay_gather_dev): the ring and its cursor against the reference's own runs
(tests/golden/replay_ring.npz, written by tests/golden/make_replay_golden.py) and against a numpy model written here from the
header's text; ranks and selection exactly, against numpy's stable argsort; sampling keys and importance weights against the
reference's formulas in float64; the k-step gather against the numpy model of tests/traj_support.py (imported, not copied).
Every test runs on the CPU harness (`-m "not gpu"`) and on the MI355X (`-m gpu`); on the harness the "device" buffers are numpy
arrays.  The harness ranks inside a tile serially: the wave ballots of the product's sort run on the GPU only, which is why the
sizes of test 3 sit around the wave (64), the sort's tile and its scan's span.

TOLERANCES (test 4).  Device and host logf / powf differ in the last bits, so keys and weights are compared with the float64
formulas within four times the error numpy's own float32 evaluation of the same formulas has on the test's inputs: that error is
the one of three float32 roundings (pow, log, divide), a second libm may differ by an ulp in each of pow and log, which at most
doubles it, and the remaining factor of two is slack.  At n = 4097, alpha 0.7, beta 0.6 the float32 evaluation is off by 2.5e-7
(keys) and 1.25e-7 (weights) relative: allowed 9.9e-7 and 5.0e-7.  The test measures the numbers again on every run and prints them."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import __graft_entry__ as ge
from tests import engines
from tests.buffers import Buf, sync
from tests.replay import GOLDEN
from tests.traj_support import OUTPUTS, assert_outputs, model_batch, out_shapes

F32, F64, U32, U8, I32 = np.float32, np.float64, np.uint32, np.uint8, np.int32
WEIGHT_TOL = 4 * 1.25e-7               # the docstring's number, for the 35 weights of the fixture


def harness_const(name):
    return int(C.c_int.in_dll(C.CDLL(ge.build_harness()), name).value)


def sort_tile():
    return harness_const("tetris_harness_sort_tile")


def sort_scan_span():
    return harness_const("tetris_harness_sort_scan_span")


def rand_bits(rng, shape, dt):
    return rng.integers(0, 256, shape).astype(U8) if dt == U8 else rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(U32)


RING_ARRAYS = ("obs", "action", "prob", "adv", "target", "reward", "done", "flags", "prio", "cursor")


class Ring:
    """A replay buffer in buffers of the engine's kind.  fill: None (zeros), an int (that byte everywhere but the cursor) or a
    Generator (random bits below max_size, zeros in the never-written rows; flags 0 / 1)."""

    def __init__(self, kind, b, capacity, k_step, fill=None, prio_only=False):
        S = b.n_players
        self.kind, self.b, self.C, self.k_step, self.max_size, self.S = kind, b, capacity, k_step, capacity - k_step, S
        shapes = dict(obs=((capacity, S, 12), U32), action=((capacity, 4), U8), prob=((capacity,), U32), adv=((capacity,), U32),
                      target=((capacity,), U32), reward=((capacity,), U32), done=((capacity,), U8), flags=((capacity,), U8),
                      prio=((self.max_size,), U32), cursor=((4,), I32))
        self.bufs = {}
        for name, (shape, dt) in shapes.items():
            if prio_only and name not in ("prio", "cursor"):
                continue
            v = np.zeros(shape, dt)
            if isinstance(fill, int) and name != "cursor":
                v = v.view(U8)
                v[...] = fill
                v = v.view(dt)
            elif fill is not None and not isinstance(fill, int) and name != "cursor":
                v = rand_bits(fill, shape, dt)
                if name == "flags":
                    v &= 1
                if name == "obs":       # words 10 / 11 as the header defines them
                    v[..., 11] = fill.integers(0, 256, shape[:2]) | (fill.integers(0, 8, shape[:2]) << 8) | (fill.integers(0, 8, shape[:2]) << 16)
                if name == "action":
                    v[:, 1], v[:, 2] = fill.integers(0, 10, capacity), fill.integers(0, 7, capacity)
                if name != "prio":
                    v[self.max_size:] = 0
            self.bufs[name] = Buf(kind, v)
        ptr = lambda n: self.bufs[n].ptr if n in self.bufs else 0                 # noqa: E731
        self.rp = b.replay(capacity, k_step, *[ptr(n) for n in RING_ARRAYS])

    def get(self):
        return {k: v.get() for k, v in self.bufs.items()}

    def put(self, name, v):
        self.bufs[name].put(v)


class RandomWindow:
    """T rows of random bits with their records, and adv / target / prio arrays"""

    def __init__(self, kind, b, T, rng):
        n, S = b.n_games, b.n_players
        self.np = dict(obs=rand_bits(rng, (T, n, S, 12), U32), action=rand_bits(rng, (T, n, 4), U8), prob=rand_bits(rng, (T, n), U32),
                       value=np.zeros((2, T, n), U32), reward=rand_bits(rng, (T, n), U32), done=rand_bits(rng, (T, n), U8),
                       adv=rand_bits(rng, (T, n), U32), target=rand_bits(rng, (T, n), U32), prio=rand_bits(rng, (T, n), U32))
        self.bufs = {k: Buf(kind, v) for k, v in self.np.items()}
        p = {k: v.ptr for k, v in self.bufs.items()}
        self.traj = b.traj(T, p["action"], p["prob"], p["value"], p["reward"], p["done"])
        self.tobs = b.traj_obs(T, p["obs"])


# ---------------------------------------------------------------- the model of add, from the header's text
def model_add(ring, max_size, win, mask, augment, prio, adv, target):
    """ring: {name: numpy} changed in place; win: the window's numpy arrays; mask [rows, N]; prio / adv / target: bool (given?)"""
    rows, N = mask.shape
    entries = []
    for g in range(N):
        run = [t * N + g for t in range(rows) if mask[t, g]]
        entries += [(e, 0) for e in run]
        if augment:
            entries += [(e, 1) for e in run]
    k = len(entries)
    idx, size, added, dropped = [int(v) for v in ring["cursor"].view(U32)]
    if idx + k > max_size:
        size, idx = idx, 0
    written = min(k, max_size)
    flat = {name: win[name].reshape((-1,) + win[name].shape[2:]) for name in ("obs", "action", "prob", "reward", "done", "adv", "target", "prio")}
    for o, (e, flag) in enumerate(entries[:written]):
        pos = idx + o
        for name in ("obs", "action", "prob", "reward", "done"):
            ring[name][pos] = flat[name][e]
        ring["adv"][pos] = flat["adv"][e] if adv else 0
        ring["target"][pos] = flat["target"][e] if target else 0
        ring["flags"][pos] = flag
        ring["prio"][pos] = flat["prio"][e] if prio else F32(2.0).view(U32)
    idx += written
    size = max(size, idx)
    ring["cursor"][:] = np.array([idx, size, (added + k) % (1 << 32), dropped + k - written], np.int64).astype(U32).view(I32)
    return k


def assert_ring(got, want, where):
    for name in want:
        assert np.array_equal(got[name], want[name]), f"{where}: '{name}' differs at {np.argwhere(got[name] != want[name])[:4].tolist()}"


def run_sample(ring, M, alpha, beta, seed, draw, rank=True):
    """-> index [M], weight [M], count, rank [max_size], key [max_size] (the last two None without rank)"""
    kind, b = ring.kind, ring.b
    index, weight, count = Buf(kind, np.full(max(M, 1), 77, I32)), Buf(kind, np.full(max(M, 1), 7.0, F32)), Buf(kind, np.full(1, -5, I32))
    rk, ky = Buf(kind, np.full(ring.max_size, -9, I32)), Buf(kind, np.full(ring.max_size, -9.0, F32))
    b.replay_sample_dev(ring.rp, M, alpha, beta, seed, draw, index.ptr, weight.ptr, count.ptr, rank=rk.ptr if rank else None,
                        key=ky.ptr if rank else None)
    sync(kind, b)
    return index.get()[:M], weight.get()[:M], int(count.get()[0]), (rk.get() if rank else None), (ky.get() if rank else None)


def run_gather(ring, index, steps, only=None, skip=None):
    kind, b = ring.kind, ring.b
    M = len(index)
    ib = Buf(kind, np.asarray(index, np.int64).astype(U32).view(I32))
    outs = {}
    for name, (shape, dt) in out_shapes(ring.S, M * steps, b.height).items():
        if (only is None or name == only) and name != skip:
            outs[name] = Buf(kind, np.full(shape, 0xA5 if dt == U8 else 0xA5A5A5A5, dt))
    b.replay_gather_dev(ring.rp, ib.ptr, M, steps, b.traj_batch(**{k: v.ptr for k, v in outs.items()}))
    sync(kind, b)
    return {k: v.get() for k, v in outs.items()}


def model_ranks(prio):
    """1 + n - rankdata(prio, 'ordinal'): numpy's stable argsort (-0.0 equals 0.0) gives the ordinal ranks"""
    n = len(prio)
    order = np.argsort(prio, kind="stable")
    ordinal = np.empty(n, np.int64)
    ordinal[order] = np.arange(1, n + 1)
    return 1 + n - ordinal


# ---------------------------------------------------------------- 1. the reference's own runs
@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
def test_ring_ranks_weights_and_update_equal_the_reference(kind):
    """tests/golden/replay_ring.npz: experience_replay(max_size=40, k_step=3) after add_samples of 11, 17, 9, 12, 30 and 5 entries
    whose states are their running numbers; one game, one episode, one mask per add.  The tag sits in word 0 of the record: the
    occupancy of column 0, which the gather hands back as the first column of `visual`."""
    z = np.load(os.path.join(GOLDEN, "replay_ring.npz"))
    cap, k_step = int(z["max_size"]), int(z["k_step"])
    T, H = int(z["adds"].max()), 20
    b = engines.make(kind, 1, 1, H)
    ring = Ring(kind, b, cap, k_step)
    assert z["cursor"].tolist() == [[11, 11], [28, 28], [37, 37], [12, 37], [30, 30], [35, 35]]
    tag = 1
    for a, n in enumerate(z["adds"].tolist()):
        t = np.arange(tag, tag + n)
        tag += n
        obs, action = np.zeros((T, 1, 1, 12), U32), np.zeros((T, 1, 4), U8)
        obs[:n, 0, 0, 0], obs[:, 0, 0, 11] = t, 7 << 8
        action[:n, 0, :3] = (t % 7)[:, None]
        reward, done, mask = np.zeros((T, 1), F32), np.zeros((T, 1), U8), np.zeros((T, 1), U8)
        reward[:n, 0], done[:n, 0], mask[:n, 0] = t % 3 - 1, t % 5 == 0, 1
        bufs = [Buf(kind, v) for v in (action, np.zeros((T, 1), F32), np.zeros((2, T, 1), F32), reward, done, obs, mask)]
        traj, tobs = b.traj(T, *[x.ptr for x in bufs[:5]]), b.traj_obs(T, bufs[5].ptr)
        b.replay_add_dev(ring.rp, traj, tobs, bufs[6].ptr, T)
        cur = ring.bufs["cursor"].get()
        assert cur[:2].tolist() == z["cursor"][a].tolist(), f"add {a}: the cursor"
        assert cur[2] == tag - 1 and cur[3] == 0
        got = ring.bufs["obs"].get()[:, 0, 0]
        lo, hi = int(z["slice_start"][a]), int(z["slice_stop"][a])
        assert np.array_equal(got[lo:hi], t), f"add {a}: the slice add_indices handed out"
    g = ring.get()
    assert np.array_equal(g["obs"][:, 0, 0], z["ring"])
    assert np.array_equal(g["done"], z["done"]) and np.array_equal(g["reward"].view(F32), z["reward"])
    assert np.array_equal(g["action"][:, :3], z["action"].astype(U8))
    assert np.array_equal(g["prio"].view(F32), np.where(np.arange(cap - k_step) < 37, F32(2.0), F32(0.0))), "every entry written got the very large prio"
    # the k-step views
    got = run_gather(ring, z["view_at"], k_step + 1)
    tags = (got["visual"][0, :, :, 0].astype(np.int64) << np.arange(H)).sum(axis=1).reshape(len(z["view_at"]), k_step + 1)
    assert np.array_equal(tags, z["view"])
    assert got["valid"].all()
    # ranks and importance weights
    n = len(z["prio"])
    assert n == int(g["cursor"][1])
    prio = g["prio"].view(F32).copy()
    prio[:n] = z["prio"]
    ring.put("prio", prio.view(U32))
    index, weight, count, rank, _ = run_sample(ring, n, float(z["alpha"]), float(z["beta"]), 3, 0)
    assert count == n and sorted(index.tolist()) == list(range(n))
    assert np.array_equal(rank[:n], z["rank"])
    w = np.empty(n, F64)
    w[index] = weight
    err = np.abs(w - z["is_weights"]) / z["is_weights"]
    print(f"is_weights: largest relative error {err.max():.3g} (allowed {WEIGHT_TOL:.3g})")
    assert err.max() <= WEIGHT_TOL
    # update_prios
    ui, up = Buf(kind, z["update_index"].astype(I32)), Buf(kind, z["update_prio"].astype(F32))
    b.replay_update_prios_dev(ring.rp, ui.ptr, up.ptr, len(z["update_index"]))
    sync(kind, b)
    # (the fixture's prios start at the reference's -1 where nothing was set; here at the 2.0 / 0.0 the adds left)
    want = prio.copy()
    want[z["update_index"]] = z["update_prio"]
    after = ring.bufs["prio"].get().view(F32)
    assert np.array_equal(after, want)
    assert np.array_equal(after[z["update_index"]], z["prio_after"][z["update_index"]])
    assert np.array_equal(after[:n].view(U32), np.where(np.isin(np.arange(n), z["update_index"]), z["prio_after"][:n], z["prio"]).view(U32))


# ---------------------------------------------------------------- 2. add against the model
MASKS = ("random", "zero", "one", "single")


def make_mask(rng, which, rows, N):
    if which == "random":
        return (rng.random((rows, N)) < 0.4).astype(U8) * rng.integers(1, 256, (rows, N)).astype(U8)      # any non-zero byte counts
    if which == "zero":
        return np.zeros((rows, N), U8)
    if which == "one":
        return np.ones((rows, N), U8)
    m = np.zeros((rows, N), U8)
    m[:, N // 2] = 1
    m[2, N // 2] = 0
    return m


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("which", MASKS)
@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("N", [1, 5, 64, 67, 257])
def test_add_equals_the_model(kind, N, S, which):
    """Three adds in a row — the case's mask, a random one, all ones — into a buffer one entry larger than the second add: the
    first may overflow (k > max_size), the second wraps wherever the first left more than one entry, the third overflows.  Every
    array of the ring and the four cursor words are compared; what no add wrote keeps the 0xA5 the buffer started with."""
    rows, k_step = 7, 2
    rng = np.random.default_rng(9000 + 10 * N + S + 100 * MASKS.index(which))
    b = engines.make(kind, N, S, 8)
    w = RandomWindow(kind, b, rows + 1, rng)
    mask2 = (rng.random((rows, N)) < 0.5).astype(U8)
    mask2[:2, 0] = 0
    wraps = overflows = 0
    for augment, given in ((False, True), (True, False), (True, True), (False, False)):
        f = 2 if augment else 1
        max_size = max(int(np.count_nonzero(mask2)) * f, 1) + 1
        ring = Ring(kind, b, max_size + k_step, k_step, fill=0xA5)
        want = ring.get()
        for a, mask in enumerate((make_mask(rng, which, rows, N), mask2, np.ones((rows, N), U8))):
            before = [int(v) for v in want["cursor"]]
            k = model_add(want, max_size, w.np, mask, augment, given, given, given)
            wraps += int(before[0] > 0 and before[0] + k > max_size and k <= max_size)
            overflows += int(k > max_size)
            opt = lambda name: w.bufs[name].ptr if given else None               # noqa: E731
            mb = Buf(kind, mask)
            b.replay_add_dev(ring.rp, w.traj, w.tobs, mb.ptr, rows, adv=opt("adv"), target=opt("target"), prio=opt("prio"), augment=augment)
            sync(kind, b)
            assert_ring(ring.get(), want, f"augment {augment}, optional arrays {given}, add {a} of {k} entries into {max_size}")
        assert want["cursor"][3] > 0, "the third add overflowed"
        for name in ("obs", "action", "prob", "done", "flags"):
            assert (want[name][max_size:].view(U8) == 0xA5).all(), "rows max_size .. C-1 are never written"
    assert overflows >= 4 and (wraps >= 1 or N == 1 or which == "zero")
    assert b.take_errors() == 0


# ---------------------------------------------------------------- 3. ranks and selection, exactly
def prio_set(rng, which, n):
    if which == "equal":                   # the state after adds: every digit of every pass in one bucket
        return np.full(n, 2.0, F32)
    if which == "bits":                    # random bits of finite floats of both signs (denormals and both zeros among them)
        v = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(U32)
        v = np.where((v >> 23) & 255 == 255, v & U32(0xBFFFFFFF), v).astype(U32)
        if n > 4:
            v[:4] = (0, 0x80000000, 0, 0x80000000)
        return v.view(F32)
    if which == "low_byte":                # values that differ only in the lowest byte
        return (U32(0x3F800000) | rng.integers(0, 256, n).astype(U32)).view(F32)
    if which == "high_byte":               # ... only in the highest (no exponent 255)
        top = rng.integers(0, 256, n).astype(U32)
        top = np.where(top & 127 == 127, top ^ 1, top).astype(U32)
        return ((top << 24) | U32(0x00345678)).view(F32)
    assert which == "repeats"              # 200 distinct values repeated: several waves of a tile hold the same digit
    return rng.random(200).astype(F32)[rng.integers(0, 200, n)]


def check_ranks_and_selection(kind, n, which, Ms=None):
    rng = np.random.default_rng(31000 + n + 7 * len(which))
    b = engines.make(kind, 1, 1, 8)
    ring = Ring(kind, b, n + 3 + 1, 1, prio_only=True)
    assert ring.max_size == n + 3
    prio = np.concatenate([prio_set(rng, which, n), np.full(3, np.inf, F32)])      # (the padding would win every rank if it were read)
    ring.put("prio", prio.view(U32))
    ring.put("cursor", np.array([n % ring.max_size, n, n, 0], I32))
    want_rank = model_ranks(prio[:n])
    alpha, beta, seed = 0.7, 0.5, 11
    keys = {}
    for M in (1, 64, n, n + 7) if Ms is None else Ms:
        for draw in (5, 5, 1 << 33):
            index, weight, count, rank, key = run_sample(ring, M, alpha, beta, seed, draw)
            c = min(M, n)
            assert count == c
            assert np.array_equal(rank[:n], want_rank), f"n={n} {which}: ranks differ at {np.argwhere(rank[:n] != want_rank)[:4].tolist()}"
            assert (rank[n:] == -9).all() and (key[n:] == -9.0).all(), "entries at and past n of the optional outputs are left alone"
            order = np.argsort(key[:n] + F32(0.0), kind="stable")[:c]                 # its own keys; -0.0 as 0.0; ties by position
            assert np.array_equal(index[:c], order), f"n={n} {which} M={M}: selection differs at {np.argwhere(index[:c] != order)[:4].tolist()}"
            assert (index[c:] == -1).all() and (weight[c:] == 0.0).all()
            assert (weight[:c] > 0).all() and (weight[:c] <= 1).all()
            if (M, draw) in keys:
                assert np.array_equal(keys[(M, draw)][0], key.view(U32)) and np.array_equal(keys[(M, draw)][1], index), "same (seed, draw): same result"
            keys[(M, draw)] = (key.view(U32), index)
        if n > 2:
            assert not np.array_equal(keys[(M, 5)][0][:n], keys[(M, 1 << 33)][0][:n]), "another draw gives other keys"
    index, weight, count, _, _ = run_sample(ring, min(n, 64), alpha, beta, seed, 5, rank=False)       # the optional outputs NULL
    assert np.array_equal(index, keys[(min(n, 64), 5)][1][:min(n, 64)]) if min(n, 64) in (1, 64, n) else True
    assert b.take_errors() == 0


def sizes_3():
    t = sort_tile()
    return [0, 1, 2, 63, 64, 65, t - 1, t, t + 1, 3 * t + 5]


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("which", ["equal", "bits", "low_byte", "high_byte", "repeats"])
@pytest.mark.parametrize("n", sizes_3())
def test_ranks_and_selection_are_exact(kind, n, which):
    check_ranks_and_selection(kind, n, which)


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
def test_ranks_and_selection_across_the_scans_carry(kind):
    span = sort_scan_span()
    assert span > 0, "the harness reports a scan that carries"
    check_ranks_and_selection(kind, (span + 1) * sort_tile() + 3, "bits", Ms=(64,))


# ---------------------------------------------------------------- 4. keys and weights against the reference's formulas
def philox_word0(seed, c0, c1, c2):
    """Philox4x32-10, key (seed, 0), counter (c0, c1, c2, 0), vectorised over c0 -> word 0 (the convention of tests/test_act_eval.py)"""
    m = np.uint64(0xFFFFFFFF)
    c0 = np.asarray(c0, np.uint64) & m
    c1, c2, c3 = np.full_like(c0, c1 & 0xFFFFFFFF), np.full_like(c0, c2 & 0xFFFFFFFF), np.zeros_like(c0)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64(0)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & m, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & m
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m, (k1 + np.uint64(0xBB67AE85)) & m
    return c0.astype(U32)


def test_philox_model_equals_the_oracles():
    from oracle import oracle as orc
    got = philox_word0(0xC0FFEE, np.array([0, 7, 0xFFFFFFFF]), 9, 0x12345678)
    assert got.tolist() == [int(orc.philox(0xC0FFEE, 0, c, 9, 0x12345678, 0)[0]) for c in (0, 7, 0xFFFFFFFF)]


UNIT_SEED, UNIT_DRAW, UNIT_AT = 0x5EED, 15587, 3538          # a counter whose Philox word is 0xFFFFFFxx: u is exactly 1


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("n,seed,draw", [(4097, 0xABCDEF, (7 << 32) | 3), (4097, UNIT_SEED, UNIT_DRAW)])
def test_keys_and_weights_equal_the_formulas(kind, n, seed, draw):
    """key = -ln(u) / rank^-alpha and weight = (rank / n)^(alpha beta) in float64, u rebuilt from a numpy Philox; the tolerances
    are four times the error of numpy's float32 evaluation of the same formulas on these inputs (the module's docstring: 2.5e-7
    and 1.25e-7 measured, 9.9e-7 and 5.0e-7 allowed).  The second case holds a position whose u is exactly 1: its key is zero."""
    rng = np.random.default_rng(4)
    b = engines.make(kind, 1, 1, 8)
    ring = Ring(kind, b, n + 3 + 2, 2, prio_only=True)
    prio = np.concatenate([rng.random(n).astype(F32), np.zeros(3, F32)])
    ring.put("prio", prio.view(U32))
    ring.put("cursor", np.array([0, n, n, 0], I32))
    alpha, beta = F32(0.7), F32(0.6)
    index, weight, count, rank, key = run_sample(ring, n, float(alpha), float(beta), seed, draw)
    assert count == n and np.array_equal(rank[:n], model_ranks(prio[:n]))
    pos = np.arange(n)
    r24 = (philox_word0(seed, pos, draw & 0xFFFFFFFF, draw >> 32) >> 8).astype(np.int64) + 1
    u = r24.astype(F64) * 2.0 ** -24
    rk = rank[:n].astype(F64)
    key64 = -np.log(u) / rk ** -F64(alpha)
    weight64 = (rk / n) ** (F64(alpha) * F64(beta))
    # the same formulas in float32, numpy's own
    key32 = -np.log(u.astype(F32)) / np.power(rk.astype(F32), -alpha)
    weight32 = np.power(rk.astype(F32) / F32(n), F32(alpha * beta))
    nz = key64 > 0
    key_meas = float(np.max(np.abs(key32[nz].astype(F64) - key64[nz]) / key64[nz]))
    weight_meas = float(np.max(np.abs(weight32.astype(F64) - weight64) / weight64))
    w = np.empty(n, F64)
    w[index] = weight
    key_err = float(np.max(np.abs(key[:n][nz].astype(F64) - key64[nz]) / key64[nz]))
    weight_err = float(np.max(np.abs(w - weight64) / weight64))
    print(f"n={n}: keys off by {key_err:.3g} (float32 model {key_meas:.3g}, allowed {4 * key_meas:.3g}); "
          f"weights off by {weight_err:.3g} (float32 model {weight_meas:.3g}, allowed {4 * weight_meas:.3g})")
    assert key_err <= 4 * key_meas and weight_err <= 4 * weight_meas
    assert (key[:n][~nz] == 0).all(), "keys that are exactly zero (u = 1) are zero"
    if seed == UNIT_SEED:
        assert r24[UNIT_AT] == 1 << 24 and key[UNIT_AT] == 0 and index[0] == np.flatnonzero(~nz)[0], "u = 1: the key is zero and wins"


# ---------------------------------------------------------------- 5. the gather
@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("S,H", [(1, 8), (2, 8), (2, 7), (1, 7)])
@pytest.mark.parametrize("M", [1, 63, 64, 65])
def test_gather_equals_the_batch_model(kind, M, S, H):
    k_step, max_size = 3, 41
    rng = np.random.default_rng(5000 + 10 * M + S + H)
    b = engines.make(kind, 3, S, H)
    ring = Ring(kind, b, max_size + k_step, k_step, fill=rng)
    g = ring.get()
    index = rng.integers(0, max_size, M).astype(np.int64)
    special = [max_size - 1, -1, max_size, 0, max_size + 5, -(1 << 31), max_size - 2]      # the first reads the unwritten rows
    for k, v in enumerate(special[:max(1, M // 4)]):
        index[M - 1 - k] = v
    assert g["flags"][:max_size].min() == 0 and g["flags"][:max_size].max() == 1, "flagged and unflagged entries"
    model = lambda x: x.reshape((x.shape[0], 1) + x.shape[1:])                    # noqa: E731  (the ring as a window of one game)
    for steps in (1, 2, k_step + 1):
        base = np.repeat(index, steps)
        at = base + np.tile(np.arange(steps), M)
        ok = (base >= 0) & (base < max_size)
        flagged = (g["flags"][np.where(ok, at, 0)] & 1).astype(np.int64)
        expanded = np.where(ok, at | (flagged << 31), -1)                        # bit 31 from the flags
        want = model_batch(model(g["obs"]), model(g["action"]), model(g["prob"]), model(g["reward"]), model(g["done"]), model(g["adv"]),
                           model(g["target"]), expanded, H)
        assert_outputs(run_gather(ring, index, steps), want, f"steps {steps}")
        if M == 65:
            for name in OUTPUTS:                                                 # each output NULL in turn, then every output but one
                assert_outputs(run_gather(ring, index, steps, skip=name), want, f"steps {steps}, {name} NULL")
            assert_outputs(run_gather(ring, index, steps, only="visual"), want, f"steps {steps}, only visual")
    assert_ring(ring.get(), g, "the gather writes nothing into the ring")
    assert b.take_errors() == 0


# ---------------------------------------------------------------- 6. argument rules and the Python layer
@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
def test_argument_rules(kind):
    pkg = ge.package()
    rng = np.random.default_rng(6)
    b = engines.make(kind, 4, 2, 8)
    ring, w = Ring(kind, b, 20, 3), RandomWindow(kind, b, 5, rng)
    mask, index, fl = Buf(kind, np.ones((5, 4), U8)), Buf(kind, np.zeros(8, I32)), Buf(kind, np.zeros(8, F32))
    count = Buf(kind, np.zeros(1, I32))
    outs = {name: Buf(kind, np.zeros(shape, dt)) for name, (shape, dt) in out_shapes(2, 8 * 4, 8).items()}
    out = b.traj_batch(**{k: v.ptr for k, v in outs.items()})

    def ring_with(**kw):
        vals = {n: ring.bufs[n].ptr for n in RING_ARRAYS}
        cap, k = kw.pop("capacity", 20), kw.pop("k_step", 3)
        vals.update(kw)
        return b.replay(cap, k, *[vals[n] for n in RING_ARRAYS])

    add = lambda bb=b, rp=ring.rp, traj=w.traj, obs=w.tobs, m=mask.ptr, rows=5, **kw: bb.replay_add_dev(rp, traj, obs, m, rows, **kw)      # noqa: E731
    sample = lambda bb=b, rp=ring.rp, M=8, i=index.ptr, wt=fl.ptr, c=count.ptr: bb.replay_sample_dev(rp, M, 0.7, 0.5, 1, 0, i, wt, c)      # noqa: E731
    update = lambda bb=b, rp=ring.rp, i=index.ptr, p=fl.ptr, M=8: bb.replay_update_prios_dev(rp, i, p, M)                                  # noqa: E731
    gather = lambda bb=b, rp=ring.rp, i=index.ptr, M=8, steps=4, o=out: bb.replay_gather_dev(rp, i, M, steps, o)                           # noqa: E731
    calls = dict(add=add, sample=sample, update=update, gather=gather)
    for name, call in calls.items():                                             # every call is fine as it stands
        call()
    sync(kind, b)
    three = engines.make(kind, 4, 3, 8)
    rows = [(name, dict(bb=three), "one or two players") for name in calls]
    rows += [(name, dict(rp=None), "replay buffer is NULL") for name in calls]
    rows += [(name, dict(rp=ring_with(k_step=-1)), "k_step must be >= 0") for name in calls]
    rows += [(name, dict(rp=ring_with(capacity=3, k_step=3)), r"must be in \[1, 2\^24\]") for name in calls]
    rows += [(name, dict(rp=ring_with(capacity=(1 << 24) + 4, k_step=3)), r"must be in \[1, 2\^24\]") for name in calls]
    rows += [(name, dict(rp=ring_with(prio=0)), "prio/cursor") for name in calls]
    rows += [(name, dict(rp=ring_with(cursor=0)), "prio/cursor") for name in calls]
    rows += [(name, dict(rp=ring_with(**{arr: 0})), "an array of the replay buffer is NULL")
             for name in ("add", "gather") for arr in ("obs", "action", "prob", "adv", "target", "reward", "done", "flags")]
    rows += [(name, dict(rp=ring_with(obs=ring.bufs["obs"].ptr + 4)), "16-byte aligned") for name in ("add", "gather")]
    rows += [("add", dict(traj=None), "the window or the mask are NULL"), ("add", dict(m=None), "the window or the mask are NULL"),
             ("add", dict(obs=None), "observation records are NULL"),
             ("add", dict(traj=b.traj(5, 0, w.bufs["prob"].ptr, w.bufs["value"].ptr, w.bufs["reward"].ptr, w.bufs["done"].ptr)), "an array of the window is NULL"),
             ("add", dict(obs=b.traj_obs(4, w.bufs["obs"].ptr)), "differ in capacity"),
             ("add", dict(rows=0), "rows outside"), ("add", dict(rows=6), "rows outside"),
             ("add", dict(rows=1 << 29), r"rows \* N must be below 2\^31")]
    rows += [("sample", dict(M=-1), "M < 0"), ("sample", dict(i=None), "index/weight/count"), ("sample", dict(wt=None), "index/weight/count"),
             ("sample", dict(c=None), "index/weight/count"),
             ("update", dict(M=-1), "M < 0"), ("update", dict(i=None), "index/prio"), ("update", dict(p=None), "index/prio"),
             ("gather", dict(M=-1), "M < 0"), ("gather", dict(i=None), "index list or the outputs"), ("gather", dict(o=None), "index list or the outputs"),
             ("gather", dict(steps=0), r"steps outside \[1, k_step \+ 1\]"), ("gather", dict(steps=5), r"steps outside \[1, k_step \+ 1\]"),
             ("gather", dict(M=1 << 30, steps=2), r"M \* steps must be below 2\^31")]
    before = ring.get()
    for name, kw, text in rows:
        with pytest.raises(pkg.TetrisError, match=text):
            calls[name](**kw)
    lib = b.lib                                                                  # an unknown flag: below the Python layer
    rc = lib.tetris_replay_add_dev(b._h, C.byref(ring.rp), C.byref(w.traj), C.byref(w.tobs), None, None, None, mask.ptr, 5, 2)
    assert rc == -1 and b"unknown flag" in lib.tetris_last_error()
    sync(kind, b)
    assert_ring(ring.get(), before, "a refused call writes nothing")


def test_split_batches_are_refused():
    pkg = ge.package()
    b = pkg.TetrisBatch(4, 2, 8, 10, lib_path=ge.build_harness(), split_side=0)
    ring = Ring("harness", b, 20, 3)
    idx, fl = Buf("harness", np.zeros(8, I32)), Buf("harness", np.zeros(8, F32))
    with pytest.raises(pkg.TetrisError, match="tetris_replay_sample_dev is not available on split batches"):
        b.replay_sample_dev(ring.rp, 8, 0.7, 0.5, 1, 0, idx.ptr, fl.ptr, idx.ptr)
    with pytest.raises(pkg.TetrisError, match="tetris_replay_update_prios_dev is not available on split batches"):
        b.replay_update_prios_dev(ring.rp, idx.ptr, fl.ptr, 8)
    with pytest.raises(pkg.TetrisError, match="tetris_replay_gather_dev is not available on split batches"):
        b.replay_gather_dev(ring.rp, idx.ptr, 8, 1, b.traj_batch())
    with pytest.raises(pkg.TetrisError, match="tetris_replay_add_dev is not available on split batches"):
        b.replay_add_dev(ring.rp, None, None, None, 1)


@pytest.mark.gpu
def test_torch_replay_round():
    """trajectory(states=True) -> advantages -> rp.add -> rp.sample -> rp.gather -> rp.update_prios at 64 two-player games, 8 rows:
    the gathered step-0 samples of unflagged entries equal tr.batch of the same window entries."""
    import torch
    pkg = ge.package()
    n, rows, H = 64, 8, 20
    b = pkg.TetrisBatch(n, 2, H, 10, device=0)
    te = importlib.import_module("drl-tetris_amd.torch_interop").TorchEnv(b)
    tr = te.trajectory(rows, states=True)
    gen = torch.Generator(device="cuda").manual_seed(5)
    for row in range(rows):
        player = torch.full((n,), row % 2, dtype=torch.uint8, device="cuda")
        tr.observe(row, player)
        ev = torch.rand(n, 4, 10, 7, device="cuda", generator=gen)
        sv = torch.rand(n, 8, device="cuda", generator=gen)
        te.step_eval(ev, sv, mode="pi", player=player, seed=1, draw=row, auto_reset=True)
        tr.record(row)
    tr.done[rows - 1] = 1                                                       # close every game's run inside the window
    _, _, closed = tr.advantages(rows, 0.99, 0.9)
    assert bool(closed.all())
    rp = te.replay(4000, k_step=2, seed=9)
    rp.add(tr, rows)                                                            # mask None: closed; augment
    assert len(rp) == 2 * rows * n and rp.dropped() == 0
    M = 96
    index, weight, count = rp.sample(M, 0.7, 0.5, draw=1, rank=True)
    assert int(count.item()) == M and len(set(index.tolist())) == M
    mb = rp.gather(index, steps=3)
    assert tuple(mb.visual.shape) == (2, M, 3, H, 10) and tuple(mb.action.shape) == (M, 3, 3) and bool(mb.valid.all())
    # ring position -> window entry: game-major, each game's run of `rows` entries followed by its mirrored copy
    pos = index.to(torch.int64)
    game, within = pos // (2 * rows), pos % (2 * rows)
    plain = within < rows
    assert bool(plain.any()) and bool((~plain).any())
    assert torch.equal(rp.flags[pos].bool(), ~plain)
    entry = ((within % rows) * n + game).to(torch.int32)
    entry = torch.where(plain, entry, entry | torch.tensor(-(1 << 31), dtype=torch.int32, device="cuda")).contiguous()
    wb = tr.batch(entry)                                                        # the mirrored ones too: bit 31
    for name in ("visual", "vector", "piece"):
        assert torch.equal(getattr(mb, name)[:, :, 0], getattr(wb, name)), name
    for name in ("action", "prob", "adv", "target", "reward", "done"):
        assert torch.equal(getattr(mb, name)[:, 0], getattr(wb, name)), name
    rp.update_prios(index, weight.clone())
    torch.cuda.synchronize()
    assert torch.equal(rp.prio[pos], weight)
    rest = torch.ones(rp.max_size, dtype=torch.bool, device="cuda")
    rest[pos] = False
    assert bool((rp.prio[rest][: len(rp) - M] == 2.0).all())
    b.close()
