"""A trajectory window's states and sample sets (include/tetris_hip.h: tetris_traj_observe_dev, tetris_traj_select_dev,
tetris_traj_batch_dev): the packed observation record, the ordered list of a mask's entries, and the expansion of a minibatch of
entries, mirrored or not, into the trainer's arrays.  Every comparison is exact equality: nothing here rounds.  The gather is
compared with a numpy model written in tests/traj_support.py from the header's text (it owes nothing to drl-tetris_amd/csrc/tetris_batch.h), the record
with tetris_observe_packed_dev, the mirror image with the reference's own recorded `aug` dictionaries and with augment_data's
output (tests/golden/traj_augment.npz, written by tests/golden/make_batch_golden.py), the selection with np.flatnonzero.  Every test
runs on the CPU harness (`-m "not gpu"`) and on the MI355X (`-m gpu`); on the harness the "device" buffers are numpy arrays."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import __graft_entry__ as ge
from tests import engines
from tests.buffers import MIRROR, Buf, sync
from tests.replay import GOLDEN
from tests.traj_support import OUTPUTS, PIECE_SWAP, Window, assert_outputs, model_batch, out_shapes, played

F32, U32, U8, I32 = np.float32, np.uint32, np.uint8, np.int32
BLOCK = 64                                                    # samples per workgroup of the batch kernel (the issue's mapping)


def select_elems():
    """mask bytes per workgroup of the selection kernels: the constant the harness exports"""
    return int(C.c_int.in_dll(C.CDLL(ge.build_harness()), "tetris_harness_select_elems").value)


def run_batch(w, index, only=None, offset=None, adv=True, target=True):
    """tetris_traj_batch_dev of the index list -> {output: numpy}; only: the one output that is not NULL; offset: (name, bytes)"""
    b, kind = w.b, w.kind
    M = len(index)
    ib = Buf(kind, np.asarray(index, np.int64).astype(U32).view(I32))
    outs = {}
    for name, (shape, dt) in out_shapes(w.S, M, b.height).items():
        if only is None or name == only:
            outs[name] = Buf(kind, np.full(shape, 0xA5 if dt == U8 else 0xA5A5A5A5, dt), offset=offset[1] if offset and offset[0] == name else 0)
    out = b.traj_batch(**{k: v.ptr for k, v in outs.items()})
    b.traj_batch_dev(w.traj, w.tobs, ib.ptr, M, out, adv=w.adv.ptr if adv else None, target=w.target.ptr if target else None)
    sync(kind, b)
    return {k: v.get() for k, v in outs.items()}


# ---------------------------------------------------------------- 1. record + expansion = the observation


CASES_1 = [(n, P, 20, False) for n in (1, 33, 64, 65, 257) for P in (1, 2)] + [(65, 2, 7, False), (65, 1, 7, False), (65, 2, 31, False),
                                                                                (33, 2, 20, True)]


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("n,P,H,colours", CASES_1)
def test_record_and_expansion_equal_the_packed_observation(kind, n, P, H, colours):
    b, rng = played(kind, n, P, H, colours, seed=100 * n + 10 * P + H)
    T = 3
    w = Window(kind, b, T)
    player = rng.integers(0, P, n).astype(U8)
    pb = Buf(kind, player)
    want = dict(zip(("visual", "vector", "piece"), b.observe_packed(None, player)))       # (tetris_observe_packed_dev behind a staged copy)
    print(f"n={n} P={P} H={H}: boards with inc_lines {int((want['vector'][..., 2] > 0).sum())}, combo_time {int((want['vector'][..., 3] > 0).sum())}, "
          f"combo_count {int((want['vector'][..., 4] > 0).sum())}")
    if n >= 33 and H == 20:
        assert want["visual"].any() and want["vector"][..., 3].any() and want["vector"][..., 4].any(), "the boards carry cells and a running combo"
    if n >= 33 and P == 2 and H == 20:
        assert want["vector"][..., 2].any(), "garbage is on its way to some board"
    for row in (0, T - 1):
        b.traj_observe_dev(w.tobs, row, pb.ptr)
        got = run_batch(w, row * n + np.arange(n))
        for k in ("visual", "vector", "piece"):
            assert np.array_equal(got[k], want[k]), f"row {row}: '{k}' differs from observe_packed"
        assert np.array_equal(got["valid"], np.ones(n, U8))
    rec = w.obs.get()
    assert not rec[1].any(), "only the rows asked for are written"
    assert np.array_equal(rec[0], rec[T - 1])
    assert b.take_errors() == 0


# ---------------------------------------------------------------- 2. the gather against the model
def index_list(rng, M, total):
    """repeats, a descending run, the very last entry, -1 entries, an out-of-range entry, bit 31 on a random half"""
    idx = rng.integers(0, total, M).astype(np.int64)
    if M >= 8:
        idx[:3] = idx[3]                                        # repeats
        idx[4:8] = np.sort(idx[4:8])[::-1]                      # descending
    idx = np.where(rng.random(M) < 0.5, idx | MIRROR, idx)
    special = [total - 1, -1 & 0xFFFFFFFF, total, (total - 1) | MIRROR, (total + 5) | MIRROR, 0x7FFFFFFF]
    for k, v in enumerate(special[:max(1, M // 4)] if M > 1 else []):
        idx[M - 1 - k] = v
    if M == 1:
        idx[0] = total - 1
    return idx


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("M", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("P,H", [(2, 20), (1, 20), (2, 7)])
def test_batch_equals_the_model(kind, M, P, H):
    rng = np.random.default_rng(7000 + 10 * M + P + H)
    n, T = 37, 5
    b = engines.make(kind, n, P, H)
    w = Window(kind, b, T, rng)
    arrays = [x.get() for x in (w.obs, w.action, w.prob, w.reward, w.done, w.adv, w.target)]
    if M == 257:       # a NaN payload and -0.0 travel bit for bit
        for buf, k in ((w.prob, 2), (w.adv, 5), (w.reward, 3)):
            v = buf.get()
            v.reshape(-1)[:2] = (0x7FC12345, 0x80000000)
            buf.put(v)
            arrays[k] = v
    idx = index_list(rng, M, T * n)
    if M == 257:
        idx[10:12] = (0, 1)
    want = model_batch(*arrays, idx, H)
    assert_outputs(run_batch(w, idx), want, "every output")
    if M in (65, 257):
        for name in OUTPUTS:                                    # every output NULL except one
            assert_outputs(run_batch(w, idx, only=name), want, f"only {name}")
        for name in ("visual", "vector", "piece", "action", "done"):      # the plain path: an output pointer one byte off
            assert_outputs(run_batch(w, idx, offset=(name, 1)), want, f"{name} offset by one byte")
        assert_outputs(run_batch(w, idx, offset=("visual", 4)), want, "visual offset by four bytes")
        want_no = model_batch(*arrays[:5], None, None, idx, H)
        assert_outputs(run_batch(w, idx, adv=False, target=False), want_no, "adv / target NULL")
    assert b.take_errors() == 0


# ---------------------------------------------------------------- 3. the mirror image against the reference
@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
def test_mirrored_samples_equal_the_references_aug_dictionaries(kind):
    """tests/golden/pygolden_worker_2p_actions_aug.npz replayed as tests/test_python_golden.py drives it: at every recorded
    get_state, observe + batch gives sd_aug_* with bit 31 set and the plain keys without, from both perspectives."""
    g = np.load(os.path.join(GOLDEN, "pygolden_worker_2p_actions_aug.npz"))
    G = {k: g[k] for k in g.files}
    n, P, steps = int(G["n_envs"]), int(G["n_players"]), int(G["steps"])
    H, W = [int(v) for v in G["game_size"]]
    assert P == 2 and bool(G["augment"])
    env_mod = importlib.import_module("drl-tetris_amd.environment")
    edt = importlib.import_module("drl-tetris_amd.data_types")
    seed = [int(G["seed0"])]
    settings = {"n_players": P, "game_size": [H, W], "pieces": G["pieces"].tolist(), "augment_data": True, "extra_rewards": bool(G["extra_rewards"]),
                "reward_ammount": (1.0, 0.25), "seed_source": lambda: seed[0], "bar_null_moves": bool(G["bar_null_moves"]) if "bar_null_moves" in G else True}
    sd_steps = G["sd_step"].tolist() if "sd_step" in G else list(range(steps))
    env = env_mod.tetris_environment_vector(n, None, settings=settings, _lib_path=ge.build_harness() if kind == "harness" else None)
    b = env.backend
    w = Window(kind, b, 2)
    checked = 0
    for it in range(steps):
        current = G["act_player"][it]
        if it in sd_steps:
            k = sd_steps.index(it)
            for persp in (current.astype(U8), (1 - current).astype(U8)):
                b.traj_observe_dev(w.tobs, 1, Buf(kind, persp).ptr)
                got = run_batch(w, np.concatenate([n + np.arange(n), (n + np.arange(n)) | MIRROR]))
                for sl in range(2):
                    who = persp if sl == 0 else 1 - persp
                    for i in range(n):
                        p = int(who[i])
                        for j, pre in ((i, "sd_"), (n + i, "sd_aug_")):
                            where = (it, sl, i, pre)
                            assert np.array_equal(got["visual"][sl, j], G[pre + "field"][k, i, p]), where
                            assert np.array_equal(got["vector"][sl, j, 5:], G[pre + "nextpiece"][k, i, p]), where
                            assert int(got["piece"][sl, j]) == int(G[pre + "piece_idx"][k, i, p]), where
                        assert int(got["vector"][sl, n + i, 0]) == int(np.ravel(G["sd_x"][k, i, p])[0]) and int(got["vector"][sl, n + i, 4]) == int(np.ravel(G["sd_combo_count"][k, i, p])[0])
                        checked += 1
        acts = [edt.action(G["act_keys"][it][i, : G["act_lens"][it][i]].tolist()) for i in range(n)]
        _, dones = env.perform_action(acts, player=[int(p) for p in current])
        seed[0] = int(G["reset_seed"][it])
        env.reset(env=[i for i, d in enumerate(dones) if d])
    assert checked >= 2 * 2 * n * 10


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
def test_select_and_batch_equal_augment_data(kind):
    """tests/golden/traj_augment.npz: process_trajectory(augment=True) of seeded episodes of lengths 1, 2 and 17 with states tagged
    by their entry number.  The episodes lie end to end in one column of a window (the tag in a record's word 0); select with
    augment + batch gives the reference's concatenation order and mirrored actions."""
    z = np.load(os.path.join(GOLDEN, "traj_augment.npz"))
    start, length = z["start"], z["length"]
    total = int(length.sum())
    assert sorted(length.tolist()) == [1, 2, 17]
    n, T = 3, total + 2
    b = engines.make(kind, n, 1)
    w = Window(kind, b, T)
    col = 1
    obs, action, prob, done = w.obs.get(), w.action.get(), w.prob.get(), w.done.get()
    obs[:total, col, 0, 0] = z["tag_in"]                                # the tagged states
    obs[:total, col, 0, 11] = 7 << 8                                    # (no next piece)
    action[:total, col, :3] = z["a_env_in"]
    prob[:total, col] = z["prob"].astype(F32).view(U32)
    done[:total, col] = z["done_in"]
    for buf, v in ((w.obs, obs), (w.action, action), (w.prob, prob), (w.done, done)):
        buf.put(v)
    for s, ln in zip(start.tolist(), length.tolist()):                  # one episode at a time, as the reference processes them
        mask = np.zeros((T, n), U8)
        mask[s:s + ln, col] = 1
        index, count = Buf(kind, np.zeros(2 * ln + 3, I32)), Buf(kind, np.zeros(1, I32))
        b.traj_select_dev(Buf(kind, mask).ptr, T, index.ptr, 2 * ln + 3, count.ptr, augment=True)
        sync(kind, b)
        assert int(count.get()[0]) == 2 * ln and np.array_equal(index.get()[2 * ln:], [-1, -1, -1])
        got = run_batch(w, index.get()[:2 * ln].view(U32))
        sl = slice(2 * s, 2 * (s + ln))
        assert np.array_equal(got["action"], z["a_env_out"][sl]), "augment_data's actions: the plain ones, then the mirrored ones"
        tags = (got["visual"][0, :, :, 0].astype(np.int64) << np.arange(20)[None, :]).sum(axis=1)       # column 0 of the plain half
        tags_m = (got["visual"][0, :, :, 9].astype(np.int64) << np.arange(20)[None, :]).sum(axis=1)     # ... is column 9 of the mirrored
        assert np.array_equal(np.where(np.arange(2 * ln) < ln, tags, tags_m), z["tag_out"][sl]), "the order of np.concatenate([x, x2])"
        assert np.array_equal(z["tag_mirrored"][sl], np.arange(2 * ln) >= ln), "bit 31 is set where the reference has the mirrored state"
        assert np.array_equal(got["prob"].view(F32), z["a_int_out"][sl, 0].astype(F32))
        assert np.array_equal(got["done"], z["d_out"][sl, 0]) and np.array_equal(got["valid"], np.ones(2 * ln, U8))
        assert np.array_equal(got["vector"][0, :ln, 5:], np.zeros((ln, 7), U8)) and np.array_equal(got["vector"][0, ln:, 5:], np.ones((ln, 7), U8))


# ---------------------------------------------------------------- 4. select against np.flatnonzero
def check_select(kind, b, rows, mask, augment, cap):
    n = b.n_games
    mb = Buf(kind, mask)
    index, count = Buf(kind, np.full(cap + 2, 77, I32)), Buf(kind, np.full(1, 77, I32))
    b.traj_select_dev(mb.ptr, rows, index.ptr, cap, count.ptr, augment=augment)
    sync(kind, b)
    k = np.flatnonzero(mask.reshape(-1)[:rows * n]).astype(np.int64)
    full = np.concatenate([k, k | MIRROR]) if augment else k
    want = np.full(cap, -1, np.int64).astype(U32)
    want[:min(cap, len(full))] = full[:cap].astype(U32)
    got = index.get()
    assert int(count.get()[0]) == len(full), (rows, n, augment, cap)
    assert np.array_equal(got[:cap].view(U32), want), (rows, n, augment, cap, np.argwhere(got[:cap].view(U32) != want)[:4].tolist())
    assert np.array_equal(got[cap:], [77, 77]), "nothing is written past cap"
    return len(full)


def masks_of(rng, rows, n):
    total = rows * n
    last = np.zeros(total, U8)
    last[-1] = 1
    other = np.where(rng.random(total) < 1 / 6, rng.integers(2, 256, total), 0).astype(U8)
    return dict(zero=np.zeros(total, U8), one=np.ones(total, U8), last=last, sixth=(rng.random(total) < 1 / 6).astype(U8), other=other)


def select_shapes():
    E = select_elems()
    return [(1, 1), (3, 65), (17, 257), (1, E - 1), (1, E), (1, E + 1), (3, E + 1)]


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("shape", range(7))
def test_select_equals_flatnonzero(kind, shape):
    rows, n = select_shapes()[shape]
    rng = np.random.default_rng(40 + shape)
    b = engines.make(kind, n, 1, 7)
    for name, mask in masks_of(rng, rows, n).items():
        mask = mask.reshape(rows, n)
        for augment in (False, True):
            full = check_select(kind, b, rows, mask, augment, rows * n * 2 + 5)              # larger than the list
            for cap in sorted({full, max(0, full - 1), full // 2, 0}):                        # equal, smaller, none
                check_select(kind, b, rows, mask, augment, cap)
    check_select(kind, b, max(1, rows - 1), masks_of(rng, rows, n)["sixth"].reshape(rows, n), True, rows * n)     # fewer rows than the mask has
    assert b.take_errors() == 0


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
def test_select_over_more_block_counts_than_one_scan_trip(kind):
    """2^21 + 4 099 mask bytes: more than 512 workgroups' counts, scanned 256 per trip"""
    E = select_elems()
    n, rows = 4099, 513
    assert rows * n >= (1 << 21) and rows * n > 256 * E + E
    rng = np.random.default_rng(44)
    b = engines.make(kind, n, 1, 7)
    mask = (rng.random((rows, n)) < 1 / 6).astype(U8)
    mask[-1, -1] = 9
    check_select(kind, b, rows, mask, True, 2 * int(np.count_nonzero(mask)))
    check_select(kind, b, rows, np.ones((rows, n), U8), False, rows * n)
    check_select(kind, b, rows, np.ones((rows, n), U8), True, rows * n + 100)


# ---------------------------------------------------------------- 5. end to end
@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
def test_actor_loop_to_minibatch(kind):
    """257 two-player games, T = 19: observe / step_eval_observe(auto_reset) / record, advantages, select(augment), batch of a
    permuted slice — against the same quantities assembled in numpy from the per-step observations and the window's arrays.  On
    the harness through the C-level calls, on the GPU through TorchEnv.trajectory(states=True)."""
    n, P, T, H = 257, 2, 19, 12
    rng = np.random.default_rng(515)
    b = engines.make(kind, n, P, height=H)
    seen = []                                                  # per row: (visual, vector, piece) of the deciding player, before the step
    if kind == "hip":
        import torch
        ti = importlib.import_module("drl-tetris_amd.torch_interop")
        te = ti.TorchEnv(b)
        tr = te.trajectory(T, states=True)
    else:
        w = Window(kind, b, T)
        o = dict(rot=Buf(kind, np.zeros(n, U8)), trans=Buf(kind, np.zeros(n, U8)), piece=Buf(kind, np.zeros(n, U8)), eval=Buf(kind, np.zeros(n, F32)),
                 value=Buf(kind, np.zeros((2, n), F32)), done=Buf(kind, np.zeros(n, U8)), lines=Buf(kind, np.zeros((P, n), U8)),
                 dead=Buf(kind, np.zeros((P, n), U8)), vis=Buf(kind, np.zeros((P, n, H, 10), U8)), vec=Buf(kind, np.zeros((P, n, 12), U8)),
                 pc=Buf(kind, np.zeros((P, n), U8)))
    for s in range(T):
        ae, se = rng.random((n, 4, 10, 7)).astype(F32), rng.standard_normal((n, 7)).astype(F32)
        player = rng.integers(0, P, n).astype(U8)
        seen.append(b.observe_packed(None, player))
        if kind == "hip":
            pt = torch.from_numpy(player).cuda()
            tr.observe(s, pt)
            te.step_eval_observe(torch.from_numpy(ae).cuda(), torch.from_numpy(se).cuda(), mode="pi", player=pt, seed=9, draw=s, auto_reset=True)
            tr.record(s)
        else:
            aeb, seb, plb = Buf(kind, ae), Buf(kind, se), Buf(kind, player)
            b.traj_observe_dev(w.tobs, s, plb.ptr)
            e = b.act_eval(aeb.ptr, o["rot"].ptr, o["trans"].ptr, n_pieces=7, state_eval=seb.ptr, n_values=7, mode="pi", player=plb.ptr, seed=9,
                           draw=s, piece=o["piece"].ptr, eval=o["eval"].ptr, value=o["value"].ptr)
            b.step_eval_observe_dev(e, o["done"].ptr, o["lines"].ptr, o["dead"].ptr, None, o["vis"].ptr, o["vec"].ptr, o["pc"].ptr, auto_reset=True)
            b.traj_record_dev(w.traj, s, e, o["done"].ptr, o["dead"].ptr)
    perm = rng.permutation(2 * T * n)
    if kind == "hip":
        adv, target, closed = tr.advantages(T, 0.98, 0.96)
        index, count = tr.select(T, augment=True)
        torch.cuda.synchronize()
        k2 = int(count.item())
        pick = index[:k2][torch.from_numpy(perm[perm < k2][:300]).cuda()].contiguous()
        got = tr.batch(pick)
        torch.cuda.synchronize()
        got = {k: (v.cpu().numpy().view(U32) if v.dtype == torch.float32 else v.cpu().numpy()) for k, v in got._asdict().items()}
        win = {k: getattr(tr, k).cpu().numpy() for k in ("action", "prob", "reward", "done", "adv", "target", "closed")}
        index, pick = index.cpu().numpy(), pick.cpu().numpy()
    else:
        closed = Buf(kind, np.zeros((T, n), U8))
        b.traj_advantages_dev(w.traj, T, 0.98, 0.96, 0.95, None, w.adv.ptr, w.target.ptr, closed.ptr)
        ib, cb = Buf(kind, np.zeros(2 * T * n, I32)), Buf(kind, np.zeros(1, I32))
        b.traj_select_dev(closed.ptr, T, ib.ptr, 2 * T * n, cb.ptr, augment=True)
        k2 = int(cb.get()[0])
        index = ib.get()
        pick = index[:k2][perm[perm < k2][:300]]
        got = run_batch(w, pick.view(U32))
        win = dict(action=w.action.get(), prob=w.prob.get(), reward=w.reward.get(), done=w.done.get(), adv=w.adv.get(), target=w.target.get(),
                   closed=closed.get())
    k = np.flatnonzero(win["closed"])
    assert 0 < len(k) < T * n and k2 == 2 * len(k), "some episodes end inside the window and some do not"
    assert np.array_equal(index[:k2].view(U32), np.concatenate([k, k | MIRROR]).astype(U32)) and np.all(index[k2:] == -1)
    assert len(pick) == 300
    e = pick.view(U32).astype(np.int64)
    at, mir = e & 0x7FFFFFFF, (e >> 31) == 1
    assert mir.any() and not mir.all()
    t_, i_ = at // n, at % n
    vis = np.stack([seen[t][0][:, i] for t, i in zip(t_, i_)], axis=1)              # [S, M, H, 10]
    vec = np.stack([seen[t][1][:, i] for t, i in zip(t_, i_)], axis=1)
    pc = np.stack([seen[t][2][:, i] for t, i in zip(t_, i_)], axis=1)
    vis = np.where(mir[None, :, None, None], vis[..., ::-1], vis)
    vec[:, :, 5:] = np.where(mir[None, :, None], 1 - vec[:, :, 5:], vec[:, :, 5:])
    pc = np.where(mir[None, :], PIECE_SWAP[pc], pc)
    a = win["action"][t_, i_]
    act = np.stack([a[:, 0], np.where(mir, 9 - a[:, 1], a[:, 1]), np.where(mir, PIECE_SWAP[a[:, 2]], a[:, 2])], axis=1).astype(U8)
    want = dict(visual=vis, vector=vec, piece=pc, action=act, done=win["done"][t_, i_], valid=np.ones(300, U8))
    want.update({f: win[f][t_, i_].view(U32) for f in ("prob", "adv", "target", "reward")})
    assert_outputs({f: np.ascontiguousarray(got[f]).view(U32) if f in ("prob", "adv", "target", "reward") else got[f] for f in got}, want, "minibatch")
    assert b.take_errors() == 0


# ---------------------------------------------------------------- 6. arguments
def test_arguments_are_checked_through_the_harness():
    pkg = ge.package()
    n, T = 5, 4
    b = engines.make("harness", n, 2)
    w = Window("harness", b, T)
    idx, cnt, mask = Buf("harness", np.zeros(8, I32)), Buf("harness", np.zeros(1, I32)), Buf("harness", np.ones((T, n), U8))
    out = b.traj_batch(valid=Buf("harness", np.zeros(8, U8)).ptr)
    bad = pytest.raises(pkg.TetrisError)
    # observe
    for row in (-1, T, T + 9):
        with pytest.raises(pkg.TetrisError, match="row"):
            b.traj_observe_dev(w.tobs, row)
    for obs in (None, b.traj_obs(T, None)):
        with pytest.raises(pkg.TetrisError, match="NULL"):
            b.traj_observe_dev(obs, 0)
    with pytest.raises(pkg.TetrisError, match="aligned"):
        b.traj_observe_dev(b.traj_obs(T, w.obs.ptr + 4), 0)
    with bad:
        b.traj_observe_dev(b.traj_obs(0, w.obs.ptr), 0)
    # select
    for kw in (dict(mask=None), dict(index=None), dict(count=None)):
        args = dict(mask=mask.ptr, index=idx.ptr, count=cnt.ptr)
        args.update(kw)
        with pytest.raises(pkg.TetrisError, match="NULL"):
            b.traj_select_dev(args["mask"], T, args["index"], 8, args["count"])
    for rows, cap in ((0, 8), (-1, 8), (T, -1)):
        with bad:
            b.traj_select_dev(mask.ptr, rows, idx.ptr, cap, cnt.ptr)
    with pytest.raises(pkg.TetrisError, match="2\\^31"):
        b.traj_select_dev(mask.ptr, (1 << 31) // n + 1, idx.ptr, 8, cnt.ptr)
    with pytest.raises(pkg.TetrisError, match="flag"):
        b._check(b.lib.tetris_traj_select_dev(b._h, mask.ptr, T, 2, idx.ptr, 8, cnt.ptr))
    # batch
    arrays = dict(action=w.action.ptr, prob=w.prob.ptr, value=w.value.ptr, reward=w.reward.ptr, done=w.done.ptr)
    for name in ("action", "prob", "reward", "done"):
        with pytest.raises(pkg.TetrisError, match="NULL"):
            b.traj_batch_dev(b.traj(T, **dict(arrays, **{name: None})), w.tobs, idx.ptr, 8, out)
    for call in (lambda: b.traj_batch_dev(None, w.tobs, idx.ptr, 8, out), lambda: b.traj_batch_dev(w.traj, None, idx.ptr, 8, out),
                 lambda: b.traj_batch_dev(w.traj, w.tobs, None, 8, out), lambda: b.traj_batch_dev(w.traj, w.tobs, idx.ptr, 8, None),
                 lambda: b.traj_batch_dev(w.traj, b.traj_obs(T, None), idx.ptr, 8, out)):
        with pytest.raises(pkg.TetrisError, match="NULL"):
            call()
    with pytest.raises(pkg.TetrisError, match="capacity"):
        b.traj_batch_dev(w.traj, b.traj_obs(T - 1, w.obs.ptr), idx.ptr, 8, out)
    with pytest.raises(pkg.TetrisError, match="aligned"):
        b.traj_batch_dev(w.traj, b.traj_obs(T, w.obs.ptr + 8), idx.ptr, 8, out)
    with bad:
        b.traj_batch_dev(w.traj, w.tobs, idx.ptr, -1, out)
    b.traj_batch_dev(w.traj, w.tobs, idx.ptr, 0, out)            # an empty list is no error
    b.traj_batch_dev(b.traj(T, **dict(arrays, value=None)), w.tobs, idx.ptr, 8, out)          # the values are not read
    # three players, split batches: as tetris_traj_record_dev
    b3 = engines.make("harness", n, 3)
    w3 = Window("harness", b3, T)
    split = pkg.TetrisBatch(n, 2, lib_path=ge.build_harness(), split_side=0)
    ws = Window("harness", split, T)
    for bb, ww in ((b3, w3), (split, ws)):
        for call in (lambda: bb.traj_observe_dev(ww.tobs, 0), lambda: bb.traj_select_dev(mask.ptr, T, idx.ptr, 8, cnt.ptr),
                     lambda: bb.traj_batch_dev(ww.traj, ww.tobs, idx.ptr, 8, out)):
            with bad:
                call()
