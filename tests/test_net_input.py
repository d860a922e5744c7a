"""The network's input side on the device (include/tetris_hip.h: tetris_net_input_dev) against the model of tests/input_support.py,
written from the header's definition: 1. the model against the reference's own two functions transcribed in torch; 2. bit equality
of the entry point with the model on hand-made records, every source, layout, element type and alignment; 3. against
tetris_traj_batch_dev and the replay's gathers on played boards; 4. the argument rules; 5. on the GPU the torch wrappers in an
actor step and a minibatch.  Every value is a small integer, exact in float32 and binary16: no tolerance anywhere.  Groups 2 to 4
run on the CPU harness (`-m "not gpu"`) and on the MI355X (`-m gpu`); on the harness the "device" buffers are numpy arrays."""
import importlib
import itertools
import re

import numpy as np
import pytest

import __graft_entry__ as ge
from tests import engines
from tests.buffers import MIRROR, Buf, sync
from tests.input_support import (BLOCK, F16, F32, I32, ITEMS, OUTPUTS, SIZES, U8, U32, InputCall, assert_outputs, model_inputs, model_stack,
                                 raw_call, ref_apply_visual_pad, ref_visual_stack)
from tests.kstep_support import RING_ARRAYS, RandomRing
from tests.traj_support import Window, model_batch, out_shapes, played

ITEM_ORDERS = [p for k in range(5) for p in itertools.permutations(ITEMS, k)]          # every subset in every order: 65


# ---------------------------------------------------------------- 1. the model against the reference's lines
def boards(H, rng):
    """uint8 [B, H, 10]: empty, full, full columns, a single cell in row 0 and in row H - 1, overhangs, random ones"""
    out = [np.zeros((H, 10), U8), np.ones((H, 10), U8)]
    cols = np.zeros((H, 10), U8)
    cols[:, [0, 4, 9]] = 1
    top, bottom = np.zeros((H, 10), U8), np.zeros((H, 10), U8)
    top[0, 3], bottom[H - 1, 9] = 1, 1
    over = np.zeros((H, 10), U8)
    over[H - 1, :] = 1
    over[H // 2, 1:9:2] = 1                                   # cells with free space below them
    over[1, 0] = 1
    out += [cols, top, bottom, over]
    out += [(rng.random((H, 10)) < p).astype(U8) for p in (0.1, 0.5, 0.9)]
    return np.stack(out)


@pytest.mark.parametrize("H", [4, 9, 20, 31])
@pytest.mark.parametrize("pad", [True, False])
def test_model_equals_the_references_pad_and_stack(H, pad):
    import torch
    f = boards(H, np.random.default_rng(100 + H))
    x = torch.from_numpy(f.astype(F32))[..., None]                                   # the cast; [N, H, W, 1]
    if pad:
        x = ref_apply_visual_pad(x)
    assert x.dtype == torch.float32
    for items in ITEM_ORDERS:
        want = ref_visual_stack(x, list(items)).numpy()                              # NHWC
        got = np.moveaxis(model_stack(f, items, pad), -3, -1).astype(F32)
        assert got.shape == want.shape and np.array_equal(got, want), f"items {items}"
    assert np.array_equal(ref_visual_stack(x).numpy(), np.moveaxis(model_stack(f, ITEMS, pad), -3, -1))      # items=None: all four


# ---------------------------------------------------------------- 2. the entry point on hand-made records
T_ROWS, N_GAMES = 2, 2 * BLOCK + 1


@pytest.fixture(scope="module")
def window_of():
    """(kind, S, H) -> a batch of N_GAMES games and a window of T_ROWS rows of random record bits — every bit of every column word,
    those at and above H included"""
    made = {}

    def get(kind, S, H):
        if (kind, S, H) not in made:
            b = engines.make(kind, N_GAMES, S, H)
            w = Window(kind, b, T_ROWS, np.random.default_rng(7 * S + H))
            obs = w.obs.get()
            assert all(((obs[..., c] >> H) != 0).any() for c in range(10)), "bits at and above H in every column word"
            made[(kind, S, H)] = (b, w, obs)
        return made[(kind, S, H)]
    return get


def index_list(rng, M, total):
    """M entries of a window of `total`: repeats, mirrored ones, -1, an entry equal to `total` and one far past it"""
    index = rng.integers(0, total, M).astype(np.int64)
    index[rng.random(M) < 0.5] |= MIRROR
    special = [total - 1, -1, total, 0, (total - 1) | MIRROR, total | MIRROR, (1 << 31) - 1, index[0]]
    for k, v in enumerate(special[:max(1, M // 2)]):
        index[M - 1 - k] = v
    return index


def window_model(obs, index, H, items, pad, dtype, channels_last):
    Tn, N, S, _ = obs.shape
    z8, z32 = np.zeros((Tn, N, 4), U8), np.zeros((Tn, N), U32)
    return model_inputs(model_batch(obs, z8, z32, z32, np.zeros((Tn, N), U8), None, None, index, H), items, pad, dtype, channels_last)


def _cases():
    """every size with both layouts and both element types; S, H, the items, the pad and the output's alignment rotate with indices of
    their own.  H = 9 with two items in binary16: a sample-slot's run of 3 x 11 x 12 x 2 bytes is no multiple of 16."""
    item_sets = [ITEMS, ("holes", "cumsum"), (), ("height",), ("shadow", "holes", "cumsum"), ("holes", "height", "shadow", "cumsum")]
    heights = [9, 20, 4, 31]
    cases = []
    for n, ((mi, M), last, dt) in enumerate(itertools.product(enumerate(SIZES), (False, True), (F32, F16))):
        cases.append((M, 1 + (n + mi) % 2, heights[(n + mi) % 4], item_sets[(n + mi) % 6], (n + mi) % 3 != 0, dt, last, (n // 2 + mi) % 2))
    for last in (False, True):
        cases.append((2 * BLOCK + 1, 2, 9, ("holes", "cumsum"), True, F16, last, 0))          # the run that is no multiple of 16 bytes
        cases.append((BLOCK + 1, 1, 31, ITEMS, True, F32, last, 1))                           # 33 rows: the tallest image
        cases.append((BLOCK + 1, 2, 20, (), False, F16, last, 1))                             # a plain float cast
    return list(dict.fromkeys(cases))


def case_id(c):
    M, S, H, items, pad, dt, last, lead = c
    return f"M{M}-S{S}-H{H}-{'_'.join(items) or 'plain'}-{'pad' if pad else 'nopad'}-{np.dtype(dt).name}-{'last' if last else 'first'}-lead{lead}"


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("case", _cases(), ids=case_id)
def test_index_form_equals_the_model(kind, case, window_of):
    M, S, H, items, pad, dt, last, lead = case
    b, w, obs = window_of(kind, S, H)
    index = index_list(np.random.default_rng(1000 + M + H), M, T_ROWS * N_GAMES)
    want = window_model(obs, index, H, items, pad, dt, last)
    assert want["valid"].min() == 0 or M == 1
    call = InputCall(kind, b, dict(obs=w.tobs, index=index), M, items, pad, dt, last, lead)
    assert_outputs(call.run(), want, "index form")
    assert b.take_errors() == 0


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
def test_each_output_alone_and_the_empty_list(kind, window_of):
    b, w, obs = window_of(kind, 2, 9)
    M = BLOCK + 1
    index = index_list(np.random.default_rng(21), M, T_ROWS * N_GAMES)
    for dt, last in ((F32, False), (F16, True)):
        want = window_model(obs, index, 9, ITEMS, True, dt, last)
        for name in OUTPUTS:
            assert_outputs(InputCall(kind, b, dict(obs=w.tobs, index=index), M, dtype=dt, channels_last=last, lead=1, only=(name,)).run(), want, f"only {name}")
            rest = tuple(o for o in OUTPUTS if o != name)
            assert_outputs(InputCall(kind, b, dict(obs=w.tobs, index=index), M, dtype=dt, channels_last=last, only=rest).run(), want, f"{name} NULL")
    empty = InputCall(kind, b, dict(obs=w.tobs, index=np.zeros(0, np.int64), m=0), 1)
    b.net_input_dev(empty.arg)                                                       # an empty list is no error
    assert empty.untouched()


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("S,H", [(1, 9), (2, 20)])
def test_row_form_equals_the_index_form(kind, S, H, window_of):
    b, w, obs = window_of(kind, S, H)
    for row, (dt, last, pad, lead) in zip(range(T_ROWS), ((F32, True, True, 1), (F16, False, False, 0))):
        index = row * N_GAMES + np.arange(N_GAMES)
        want = window_model(obs, index, H, ("shadow", "cumsum", "holes"), pad, dt, last)
        assert want["valid"].all()
        call = InputCall(kind, b, dict(obs=w.tobs, index=None, row=row), N_GAMES, ("shadow", "cumsum", "holes"), pad, dt, last, lead)
        assert_outputs(call.run(), want, f"row {row}")


def ring_model(g, index, rows, max_size, H, items, pad, dtype, channels_last):
    """the replay form from the ring's arrays: sample j n + i is position index[j] + rows[i], mirrored by its flag"""
    n = len(rows)
    base = np.repeat(np.asarray(index, np.int64), n)
    at = base + np.tile(np.asarray(rows), len(index))
    ok = (base >= 0) & (base < max_size)
    flagged = (g["flags"][np.where(ok, at, 0)] & 1).astype(np.int64)
    expanded = np.where(ok, at | (flagged << 31), -1)
    obs = g["obs"][:, None]                                                         # the ring as a window of one game
    Cn = obs.shape[0]
    z8, z32 = np.zeros((Cn, 1, 4), U8), np.zeros((Cn, 1), U32)
    return model_inputs(model_batch(obs, z8, z32, z32, np.zeros((Cn, 1), U8), None, None, expanded, H), items, pad, dtype, channels_last)


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("M,S,H", [(1, 1, 9), (BLOCK - 1, 2, 9), (BLOCK + 1, 2, 20), (2 * BLOCK + 1, 1, 7)])
def test_replay_form_equals_the_model(kind, M, S, H):
    k_step, max_size = 3, 41
    rng = np.random.default_rng(300 + M)
    b = engines.make(kind, 3, S, H)
    ring = RandomRing(kind, b, max_size + k_step, k_step, rng)
    g = ring.np
    index = rng.integers(0, max_size, M).astype(np.int64)
    for k, v in enumerate([max_size - 1, -1, max_size, 0, max_size + 5][:max(1, M // 3)]):
        index[M - 1 - k] = v
    assert g["flags"][:max_size].min() == 0 and g["flags"][:max_size].max() == 1, "flagged and unflagged entries"
    for n, (source, rows) in enumerate([(dict(steps=1), [0]), (dict(steps=k_step + 1), [0, 1, 2, 3]), (dict(step_mask=0b1010), [1, 3]),
                                        (dict(step_mask=0b0111), [0, 1, 2])]):
        dt, last, pad, items = (F32, F16)[n % 2], n // 2 == 1, n != 2, (ITEMS, ("height", "holes"))[n % 2]
        want = ring_model(g, index, rows, max_size, H, items, pad, dt, last)
        call = InputCall(kind, b, dict(replay=ring.rp, index=index, **source), M * len(rows), items, pad, dt, last, lead=n % 2)
        assert_outputs(call.run(), want, f"{source}")
    assert all(np.array_equal(ring.bufs[name].get(), g[name]) for name in RING_ARRAYS), "the call writes nothing into the ring"
    assert b.take_errors() == 0


# ---------------------------------------------------------------- 3. against the paths that exist
def batch_outputs(kind, b, call, n):
    """visual, vector, piece, valid of a tetris_traj_batch_dev / tetris_replay_gather*_dev call for n samples: call(out struct)"""
    shapes = out_shapes(b.n_players, n, b.height)
    bufs = {k: Buf(kind, np.zeros(*shapes[k])) for k in ("visual", "vector", "piece", "valid")}
    call(b.traj_batch(**{k: v.ptr for k, v in bufs.items()}))
    sync(kind, b)
    return {k: v.get() for k, v in bufs.items()}


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("H", [20, 8])
def test_played_boards_equal_batch_and_gather(kind, H):
    """8 two-player games, 30 steps played, then 6 rows observed into a window with steps between them"""
    n, P, rows = 8, 2, 6
    b, rng = played(kind, n, P, H, False, 40 + H)
    w = Window(kind, b, rows)
    for row in range(rows):
        player = rng.integers(0, P, n).astype(U8)
        pb = Buf(kind, player)
        b.traj_observe_dev(w.tobs, row, pb.ptr)
        done = b.step_rt(rng.integers(0, 4, n).astype(U8), rng.integers(0, 10, n).astype(U8), player, ms=400)
        idx = np.flatnonzero(done).astype(I32)
        if len(idx):
            b.reset(idx, np.arange(len(idx)) + 100 * row)
    assert (w.obs.get()[..., :10] != 0).any(), "the boards are not empty"
    # a window's index list, mirrored entries and non-entries included, against batch's uint8 outputs
    index = index_list(rng, 3 * BLOCK + 5, rows * n)
    ib = Buf(kind, index.astype(U32).view(I32))
    got = batch_outputs(kind, b, lambda out: b.traj_batch_dev(w.traj, w.tobs, ib.ptr, len(index), out), len(index))
    assert got["visual"].any() and got["valid"].min() == 0
    for dt, last, items in ((F32, False, ITEMS), (F16, True, ("holes", "shadow"))):
        assert_outputs(InputCall(kind, b, dict(obs=w.tobs, index=index), len(index), items, True, dt, last).run(),
                       model_inputs(got, items, True, dt, last), "inputs(index) against batch(index)")
    # a row against its index list
    for r in (0, rows - 1):
        by_row = InputCall(kind, b, dict(obs=w.tobs, index=None, row=r), n).run()
        by_index = InputCall(kind, b, dict(obs=w.tobs, index=r * n + np.arange(n)), n).run()
        assert_outputs(by_row, by_index, f"inputs(row={r})")
        assert by_row["valid"].all()
    # the ring after add: a count, a step list; flagged (mirrored) positions and indices at and past max_size
    k_step, max_size = 2, 2 * rows * n + 7
    ring = RandomRing(kind, b, max_size + k_step, k_step, rng)
    for name in RING_ARRAYS:
        ring.bufs[name].put(0)
    mask = Buf(kind, np.ones((rows, n), U8))
    b.replay_add_dev(ring.rp, w.traj, w.tobs, mask.ptr, rows, adv=w.adv.ptr, target=w.target.ptr, augment=True)
    sync(kind, b)
    flags = ring.bufs["flags"].get()
    assert int(ring.bufs["cursor"].get()[1]) == 2 * rows * n and flags[:max_size].min() == 0 and flags[:max_size].max() == 1
    M = BLOCK + 3
    rindex = rng.integers(0, 2 * rows * n - k_step, M).astype(np.int64)
    rindex[:4] = [int(np.flatnonzero(flags)[0]), max_size, max_size + 1, -1]
    rb = Buf(kind, rindex.astype(U32).view(I32))
    for source, steps, call in (
            (dict(steps=k_step + 1), k_step + 1, lambda out: b.replay_gather_dev(ring.rp, rb.ptr, M, k_step + 1, out)),
            (dict(step_mask=0b101), 2, lambda out: b.replay_gather_steps_dev(ring.rp, rb.ptr, M, 0b101, out))):
        got = batch_outputs(kind, b, call, M * steps)
        assert got["visual"].any() and got["valid"].min() == 0 and got["valid"].max() == 1
        assert_outputs(InputCall(kind, b, dict(replay=ring.rp, index=rindex, **source), M * steps, ITEMS, True, F32, True).run(),
                       model_inputs(got, ITEMS, True, F32, True), f"Replay.inputs against gather, {source}")
    assert b.take_errors() == 0


# ---------------------------------------------------------------- 4. the argument rules
@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
def test_argument_rules(kind):
    rng = np.random.default_rng(4)
    n, Tn, H = 4, 3, 8
    b = engines.make(kind, n, 2, H)
    w = Window(kind, b, Tn, rng)
    ring = RandomRing(kind, b, 20, 3, rng)
    index = np.arange(8)

    def ring_with(**kw):
        vals = {name: ring.bufs[name].ptr for name in RING_ARRAYS}
        cap, k = kw.pop("capacity", 20), kw.pop("k_step", 3)
        vals.update(kw)
        return b.replay(cap, k, *[vals[name] for name in RING_ARRAYS])

    def refused(text, source, n_out=8, bb=None, **kw):
        call = InputCall(kind, bb or b, source, n_out, **kw)
        return call, text

    win = dict(obs=w.tobs, index=index)
    rows = [
        refused("obs and replay are both given", dict(obs=w.tobs, replay=ring.rp, index=index)),
        refused("observation records are NULL", dict(index=index)),
        refused("observation records are NULL", dict(obs=b.traj_obs(Tn, None), index=index)),
        refused("16-byte aligned", dict(obs=b.traj_obs(Tn, w.obs.ptr + 4), index=index)),
        refused("between 1 and 2\\^31 - 1 entries", dict(obs=b.traj_obs(0, w.obs.ptr), index=index)),
        refused("between 1 and 2\\^31 - 1 entries", dict(obs=b.traj_obs(1 << 29, w.obs.ptr), index=index)),
        refused("row outside the window", dict(obs=w.tobs, index=None, row=-1), n),
        refused("row outside the window", dict(obs=w.tobs, index=None, row=Tn), n),
        refused("the row form takes M = N samples", dict(obs=w.tobs, index=None, row=0, m=n - 1), n),
        refused("the row form takes M = N samples", dict(obs=w.tobs, index=None, row=0, m=n + 1), n + 1),
        refused("M < 0", dict(obs=w.tobs, index=index, m=-1)),
        # the replay form: the gather's rules
        refused("M < 0", dict(replay=ring.rp, index=index, m=-1)),
        refused("index list or the outputs", dict(replay=ring.rp, index=None, m=8)),
        refused("steps outside \\[1, k_step \\+ 1\\]", dict(replay=ring.rp, index=index, steps=0)),
        refused("steps outside \\[1, k_step \\+ 1\\]", dict(replay=ring.rp, index=index, steps=5)),
        refused("step_mask has a bit above k_step", dict(replay=ring.rp, index=index, step_mask=0b10001)),
        refused("M \\* steps must be below 2\\^31", dict(replay=ring.rp, index=index, m=1 << 30, steps=2)),
        refused("k_step must be >= 0", dict(replay=ring_with(k_step=-1), index=index)),
        refused("must be in \\[1, 2\\^24\\]", dict(replay=ring_with(capacity=3, k_step=3), index=index)),
        refused("prio/cursor", dict(replay=ring_with(prio=0), index=index)),
        refused("an array of the replay buffer is NULL", dict(replay=ring_with(obs=0), index=index)),
        refused("an array of the replay buffer is NULL", dict(replay=ring_with(flags=0), index=index)),
        refused("16-byte aligned", dict(replay=ring_with(obs=ring.bufs["obs"].ptr + 8), index=index)),
        # three players
        refused("one or two players", win, bb=engines.make(kind, n, 3, H)),
    ]
    for call, text in rows:
        rc, msg = raw_call(call.b, call.arg)
        assert rc == -1 and re.search(text, msg), f"expected '{text}', got rc {rc}: {msg}"
        assert call.untouched(), f"'{text}': a refused call wrote something"
    # the struct's own fields, below the Python layer's checks
    good = InputCall(kind, b, win, 8)

    def with_fields(**kw):
        call = InputCall(kind, b, win, 8)
        for k, v in kw.items():
            if k == "items":
                for i, code in enumerate(v):
                    call.arg.items[i] = code
            else:
                setattr(call.arg, k, v)
        return call
    for text, kw in (("n_items must be in \\[0, 4\\]", dict(n_items=5)), ("n_items must be in \\[0, 4\\]", dict(n_items=-1)),
                     ("unknown item code", dict(items=[1, 0, 3, 4])), ("unknown item code", dict(items=[5, 2, 3, 4])),
                     ("an item code is named twice", dict(items=[1, 2, 3, 1])), ("an item code is named twice", dict(n_items=2, items=[3, 3])),
                     ("unknown flag", dict(flags=8)), ("unknown flag", dict(flags=4 | 16)),
                     ("aligned to their element type", dict(d_visual=good.out["visual"].ptr + 2)),
                     ("aligned to their element type", dict(flags=4 | 1, d_vector=good.out["vector"].ptr + 1))):
        call = with_fields(**kw)
        rc, msg = raw_call(b, call.arg)
        assert rc == -1 and re.search(text, msg), f"expected '{text}', got rc {rc}: {msg}"
        assert call.untouched(), f"'{text}': a refused call wrote something"
    rc, msg = raw_call(b, None)
    assert rc == -1 and "argument struct is NULL" in msg
    pkg = ge.package()
    with pytest.raises(pkg.TetrisError, match="argument struct is NULL"):
        b.net_input_dev(None)
    assert_outputs(good.run(), window_model(w.obs.get(), index, H, ITEMS, True, F32, False), "the call is fine as it stands")


def test_split_batches_are_refused():
    pkg = ge.package()
    split = pkg.TetrisBatch(4, 2, 8, 10, lib_path=ge.build_harness(), split_side=0)
    w = Window("harness", split, 2)
    call = InputCall("harness", split, dict(obs=w.tobs, index=np.arange(4)), 4)
    with pytest.raises(pkg.TetrisError, match="tetris_net_input_dev is not available on split batches"):
        split.net_input_dev(call.arg)
    assert call.untouched()


# ---------------------------------------------------------------- 5. the torch wrappers (GPU only)
@pytest.mark.gpu
def test_torch_wrappers_in_an_actor_step_and_a_minibatch():
    """TorchEnv.net_input, Trajectory.inputs and Replay.inputs on torch tensors: equal to the model applied to the uint8 paths, the
    shapes and strides a torch convolution accepts — channels_last included —, and the same storage for a second call."""
    import torch
    pkg = ge.package()
    n, rows, H = 64, 6, 20
    b = pkg.TetrisBatch(n, 2, H, 10, device=0)
    te = importlib.import_module("drl-tetris_amd.torch_interop").TorchEnv(b)
    tr = te.trajectory(rows, states=True)
    gen = torch.Generator(device="cuda").manual_seed(3)
    torch.manual_seed(3)
    convs = {cl: torch.nn.Sequential(torch.nn.Conv2d(5, 8, 3, padding=1), torch.nn.ReLU(), torch.nn.Conv2d(8, 4, 3)).cuda() for cl in (False, True)}
    convs[True] = convs[True].to(memory_format=torch.channels_last)
    host = lambda t: t.cpu().numpy()                                                 # noqa: E731

    def check(got, batch, items, pad, dt, cl, where):
        torch.cuda.synchronize()
        want = model_inputs({k: host(getattr(batch, k)) for k in ("visual", "vector", "piece", "valid")}, items, pad, dt, False)
        lead = want["valid"].shape
        names = dict(zip(OUTPUTS, got))
        assert names["visual"].shape == want["visual"].shape, where
        assert_outputs({k: host(v.contiguous()).reshape(want[k].shape) for k, v in names.items()}, want, where)
        if cl:
            k = 1 + len(lead)
            assert names["visual"].permute(*range(k), k + 1, k + 2, k).is_contiguous(), "a permuted view of [.., Hp, Wp, C]"

    for row in range(rows):                                                          # the actor loop
        player = torch.full((n,), row % 2, dtype=torch.uint8, device="cuda")
        tr.observe(row, player)
        cl = row % 2 == 1
        visual, vector, piece, valid = tr.inputs(row=row, channels_last=cl)
        assert visual.shape == (2, n, 5, H + 2, 12) and vector.shape == (2, n, 12) and visual.dtype == torch.float32
        x = visual[0]
        assert x.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format)
        y = convs[cl](x)
        assert y.shape == (n, 4, H, 10)
        uvis, uvec, upiece = (t.clone() for t in te.observe(player))
        alone = te.net_input(player, channels_last=cl)
        if row == rows - 1:
            torch.cuda.synchronize()
            for a_, b_ in zip(alone, (visual, vector, piece, valid)):
                assert torch.equal(a_, b_), "net_input equals observe(row) + inputs(row=row)"
            assert torch.equal(alone[0][:, :, 0, 1:H + 1, 1:11], uvis.to(torch.float32)) and torch.equal(alone[1], uvec.to(torch.float32))
            assert torch.equal(alone[2], upiece) and bool(alone[3].all())
            again = te.net_input(player, channels_last=cl)
            assert all(a_.data_ptr() == b_.data_ptr() for a_, b_ in zip(alone, again)), "reused storage"
        ev = torch.rand(n, 4, 10, 7, device="cuda", generator=gen) + y.mean().detach() * 0
        te.step_eval(ev, torch.rand(n, 8, device="cuda", generator=gen), mode="pi", player=player, seed=1, draw=row, auto_reset=True)
        tr.record(row)
    tr.done[rows - 1] = 1
    tr.advantages(rows, 0.99, 0.9)
    index, count = tr.select(rows, augment=True)
    torch.cuda.synchronize()
    assert int(count.item()) == 2 * rows * n
    pick = index[torch.randperm(2 * rows * n, device="cuda", generator=gen)[:96]].contiguous()
    pick[0] = -1
    for items, pad, dt, cl in ((ITEMS, True, torch.float32, True), (("holes", "cumsum"), True, torch.float16, False), ((), False, torch.float32, False)):
        got = tr.inputs(pick, items=items, pad=pad, dtype=dt, channels_last=cl)
        check(got, tr.batch(pick), items, pad, F16 if dt == torch.float16 else F32, cl, f"Trajectory.inputs {items}")
        assert all(a_.data_ptr() == b_.data_ptr() for a_, b_ in zip(got, tr.inputs(pick, items=items, pad=pad, dtype=dt, channels_last=cl)))
    visual = tr.inputs(pick, channels_last=True)[0]                                  # a minibatch through the conv, forward and backward
    loss = convs[True](visual[0]).square().mean() + convs[False](tr.inputs(pick)[0][1]).square().mean()
    loss.backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for c in convs.values() for p in c.parameters())
    rp = te.replay(4000, k_step=2, seed=9)
    rp.add(tr, rows)
    rindex, _, _ = rp.sample(40, 0.7, 0.5, draw=1)
    rindex = rindex.clone()
    rindex[1] = rp.max_size
    for steps, cl in ((3, True), ((0, 2), False), (1, False)):
        got = rp.inputs(rindex, steps=steps, channels_last=cl)
        K = steps if isinstance(steps, int) else len(steps)
        assert got[0].shape == (2, 40, K, 5, H + 2, 12) and got[1].shape == (2, 40, K, 12) and got[3].shape == (40, K)
        check(got, rp.gather(rindex, steps=steps), ITEMS, True, F32, cl, f"Replay.inputs steps {steps}")
        assert all(a_.data_ptr() == b_.data_ptr() for a_, b_ in zip(got, rp.inputs(rindex, steps=steps, channels_last=cl)))
    torch.cuda.synchronize()
    assert b.take_errors() == 0
    b.set_stream(None, external=False)
    b.close()
