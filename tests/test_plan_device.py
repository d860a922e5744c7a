"""Planning on the device (include/tetris_hip.h: tetris_action_lists_dev, tetris_simulate_lists_dev, tetris_step_lists_dev)
against the host path it replaces: tetris_environment_vector.get_actions (backend lists + data_types.action_list),
simulate_all_actions, perform_action (step_keys), the oracle, and the reference's own Python (pygolden fixture).  Every test
runs on the CPU harness (`-m "not gpu"`) and on the MI355X (`-m gpu`); on the harness the "device" buffers are numpy arrays."""
import importlib
import os

import numpy as np
import pytest

import __graft_entry__ as ge
from oracle import oracle as orc
from tests import engines, replay
from tests.buffers import Buf
from tests.plan_support import _bits, _device_lists, _lists, _numpy_deltas, _plan_env, _scramble, _simulate
from tests.replay import GOLDEN

env_mod = importlib.import_module("drl-tetris_amd.environment")
edt = importlib.import_module("drl-tetris_amd.data_types")
ERR_LISTS = 8


def _n(kind, cpu, gpu):
    return gpu if kind == "hip" else cpu


def _want_lists(b, player, keep_null, max_lists=128):
    """tetris_environment_vector.get_actions: the backend's lists + data_types.action_list.  The backend lists are taken from
    the CPU harness holding the same games (a snapshot moves unchanged), whose get_actions the golden traces check."""
    h = engines.make("harness", b.n_games, b.n_players, height=b.height, pieces=b.piece_map.tolist())
    h.restore(b.snapshot())
    raw = h.get_actions(None, player, max_lists=max_lists, max_keys=64)
    return [[list(a) for a in edt.action_list(l, remove_null=not keep_null)] for l in raw]


def _check_lists(kind, b, player, keep_null, where):
    cnt, lens, keys, _ = _device_lists(kind, b, player, keep_null)
    c, ln, k = cnt.get(), lens.get(), keys.get()
    want = _want_lists(b, player, keep_null)
    for i in range(b.n_games):
        got = [k[i, j, : ln[i, j]].tolist() for j in range(c[i])]
        assert got == want[i], f"{where}: game {i} ({c[i]} lists, want {len(want[i])})"
    assert (c >= 1).all()
    assert b.take_errors() == 0


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("P", [1, 2])
@pytest.mark.parametrize("steps", [0, 12, 40])
def test_action_lists_match_get_actions(kind, P, steps):
    n = _n(kind, 48, 4096)
    b = engines.make(kind, n, P, seeds=orc.episode_seed(np.arange(n), 3))
    _scramble(b, steps, P)
    rng = np.random.default_rng(steps)
    player = rng.integers(0, P, n)
    for keep_null in (False, True):
        _check_lists(kind, b, player, keep_null, f"P={P} steps={steps} keep_null={keep_null}")


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
def test_get_actions_matches_harness_in_every_chunk(kind):
    """tetris_get_actions works through its games 1 024 at a time (four chunks on the GPU); every game's lists must be its own,
    those from game 1 024 on included."""
    n = _n(kind, 48, 4096)
    b = engines.make(kind, n, 2, seeds=orc.episode_seed(np.arange(n), 13))
    _scramble(b, 30, 2)
    player = np.random.default_rng(13).integers(0, 2, n)
    h = engines.make("harness", n, 2, height=b.height, pieces=b.piece_map.tolist())
    h.restore(b.snapshot())
    got = b.get_actions(None, player, max_lists=128, max_keys=64)
    want = h.get_actions(None, player, max_lists=128, max_keys=64)
    for i in range(n):
        assert got[i] == want[i], f"game {i}: {len(got[i])} lists, want {len(want[i])}"


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("P", [3, 4])
def test_action_lists_three_and_four_players(kind, P):
    n = _n(kind, 40, 384)
    b = engines.make(kind, n, P, seeds=orc.episode_seed(np.arange(n), 5))
    _scramble(b, 15, P)
    player = np.random.default_rng(P).integers(0, P, n)
    for keep_null in (False, True):
        _check_lists(kind, b, player, keep_null, f"P={P} keep_null={keep_null}")


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
def test_action_lists_height_22(kind):
    n = _n(kind, 40, 4096)
    b = engines.make(kind, n, 2, height=22, seeds=orc.episode_seed(np.arange(n), 9))
    _scramble(b, 25, 2)
    player = np.arange(n) % 2
    for keep_null in (False, True):
        _check_lists(kind, b, player, keep_null, f"H=22 keep_null={keep_null}")


_TRACE_BOARDS = {}


def _trace_boards(name, every=9, max_events=1500):
    """Snapshots of the one game of a golden trace (tall stacks, holes, overhangs), replayed through the CPU harness: one
    every `every` events while the round is on.  Blobs move between the harness and the GPU library unchanged."""
    if name not in _TRACE_BOARDS:
        t = replay.load_trace(name)
        P, H, pieces = int(t["n_players"]), int(t["height"]), t["pieces"].tolist()
        kinds, seeds, players, keys, lens = t["ev_kind"], t["ev_seed"], t["ev_player"], t["ev_keys"], t["ev_len"]
        eng, blobs = None, []
        for e in range(min(len(kinds), max_events)):
            k = int(kinds[e])
            if k == 2:
                eng = engines.make("harness", 1, P, height=H, pieces=pieces, seeds=int(seeds[e]))
            elif k == 0:
                eng.reset(None, seeds=int(seeds[e]))
            else:
                K = np.zeros((1, P, keys.shape[1]), np.uint8)
                L = np.ones((1, P), np.uint8)
                K[0, players[e]] = keys[e]
                L[0, players[e]] = lens[e]
                eng.make_actions(K, L)
                eng.finish_actions(int(t["ms"]))
            if e % every == 0 and not eng.observe()[1][0]:
                blobs.append(eng.snapshot()[0])
        _TRACE_BOARDS[name] = (P, H, pieces, np.array(blobs))
    return _TRACE_BOARDS[name]


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("name", ["garbage_flood_2p", "garbage_flood_2p_12", "greedy_2p", "greedy_2p_b", "greedy_1p"])
def test_action_lists_on_trace_boards(kind, name):
    P, H, pieces, blobs = _trace_boards(name)
    assert len(blobs) > 20
    b = engines.make(kind, len(blobs), P, height=H, pieces=pieces)
    b.restore(blobs)
    occ = b.observe()[0]["field"][:, :, :H].any(axis=3)                  # [n, P, H] rows holding a square
    heights = H - np.where(occ.any(axis=2), occ.argmax(axis=2), H)
    assert heights.max() >= H // 2, "the trace should reach tall stacks"
    for player in range(P):
        for keep_null in (False, True):
            _check_lists(kind, b, np.full(len(blobs), player), keep_null, f"{name} player {player} keep_null={keep_null}")


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("P", [1, 2])
def test_simulate_matches_simulate_all_actions(kind, P):
    n = 64
    env = env_mod.tetris_environment_vector(n, None, settings={"n_players": P, "game_size": [20, 10], "seed_source": lambda: 11},
                                            _lib_path=ge.build_harness() if kind == "harness" else None)
    b = env.backend
    b.reset(None, seeds=orc.episode_seed(np.arange(n), 1))
    _scramble(b, 14, P)
    player = (np.arange(n) + 1) % P
    cnt, lens, keys, pl = _device_lists(kind, b, player, False)
    c = cnt.get()
    for fin in (False, True):
        blob = b.snapshot()
        cols, done, lines, dead = _simulate(kind, b, cnt, lens, keys, pl, fin)
        assert np.array_equal(b.snapshot(), blob), "simulate wrote the batch's state"
        sims = env.simulate_all_actions(player=player.tolist(), finalize=fin)
        for i in range(n):
            assert len(sims[i]) == c[i]
            for k, st in enumerate(sims[i]):
                for p in range(P):
                    want = np.asarray(st[p]["field"]).reshape(20, 10) > 0
                    assert np.array_equal(_bits(cols[k, p, :, i], 20), want), (fin, i, k, p)
        if not fin:                              # done / lines / dead are only written with finalize
            assert (done == 77).all() and (lines == 77).all() and (dead == 77).all()
        # nothing is written past each game's count
        beyond = np.arange(128)[:, None] >= c[None, :]
        assert not cols.transpose(0, 3, 1, 2)[beyond].any()


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("P", [1, 2])
def test_simulate_matches_oracle(kind, P):
    """The oracle (C restatement) with one game per list: copy_from, make_actions, finish_actions; fields, done, lines, dead."""
    n = _n(kind, 48, 4096)
    seeds = orc.episode_seed(np.arange(n), 0)
    dev = engines.make(kind, n, P, seeds=seeds)
    ref = orc.OracleBatch(n, P, 20, 10, seeds=seeds)
    rng = np.random.default_rng(P)
    for s in range(30):
        rot, trans = rng.integers(0, 4, n).astype(np.uint8), rng.integers(0, 10, n).astype(np.uint8)
        d = dev.step_rt(rot, trans, player=s % P)
        assert np.array_equal(d, ref.step_rt(rot, trans, player=s % P))
        idx = np.nonzero(d)[0].astype(np.int32)
        if len(idx):
            dev.reset(idx, orc.episode_seed(idx, s + 1))
            ref.reset(idx, orc.episode_seed(idx, s + 1))
    engines.assert_same_state(dev, ref, where="before planning")
    player = rng.integers(0, P, n)
    cnt, lens, keys, pl = _device_lists(kind, dev, player, False)
    c, ln, k = cnt.get(), lens.get(), keys.get()
    T = int(c.sum())
    src = np.repeat(np.arange(n), c).astype(np.int32)
    lk = np.concatenate([np.arange(x) for x in c])
    K = np.zeros((T, P, 48), np.uint8)
    Ls = np.ones((T, P), np.uint8)
    K[np.arange(T), player[src]] = k[src, lk]
    Ls[np.arange(T), player[src]] = ln[src, lk]
    for fin in (False, True):
        blob = dev.snapshot()
        cols, done, lines, dead = _simulate(kind, dev, cnt, lens, keys, pl, fin)
        assert np.array_equal(dev.snapshot(), blob)
        one = orc.OracleBatch(T, P, 20, 10)
        one.copy_from(ref, dst_idx=np.arange(T, dtype=np.int32), src_idx=src)
        one.make_actions(K, Ls)
        if fin:
            want_done = one.finish_actions(400)
        rec = one.observe()[0]
        got = _bits(cols[lk, :, :, src], 20)                                 # [T, P, 20, 10]
        assert np.array_equal(got, rec["field"][:, :, :20] > 0)
        if fin:
            assert np.array_equal(done[lk, src], want_done)
            assert np.array_equal(lines[lk, :, src], rec["reward"])
            assert np.array_equal(dead[lk, :, src], rec["dead"])


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
def test_simulate_reproduces_reference_python(kind):
    """pygolden_worker_2p_actions_aug.npz (the reference's own Python over its compiled backend): at every sim_step the
    afterstates of game 0 (sim_n_*, sim_fields_*) for both finalize values."""
    G = dict(np.load(os.path.join(GOLDEN, "pygolden_worker_2p_actions_aug.npz")))
    n, P, steps = int(G["n_envs"]), int(G["n_players"]), int(G["steps"])
    H, W = [int(v) for v in G["game_size"]]

    class Seeds:
        next = int(G["seed0"])

        def __call__(self):
            return int(self.next)

    seeds = Seeds()
    settings = {"n_players": P, "game_size": [H, W], "pieces": G["pieces"].tolist(), "augment_data": bool(G["augment"]),
                "extra_rewards": bool(G["extra_rewards"]), "reward_ammount": (1.0, 0.25), "seed_source": seeds}
    env = env_mod.tetris_environment_vector(n, None, settings=settings, _lib_path=ge.build_harness() if kind == "harness" else None)
    b = env.backend
    sim_k = 0
    for it in range(steps):
        current = G["act_player"][it]
        if sim_k < len(G["sim_step"]) and int(G["sim_step"][sim_k]) == it:
            cnt, lens, keys, pl = _device_lists(kind, b, current.astype(np.uint8), False)
            for fin in (1, 0):
                cols = _simulate(kind, b, cnt, lens, keys, pl, bool(fin))[0]
                c0 = int(cnt.get()[0])
                assert c0 == int(G[f"sim_n_{fin}"][sim_k])
                for a in range(c0):
                    for p in range(P):
                        assert np.array_equal(_bits(cols[a, p, :, 0], H), G[f"sim_fields_{fin}"][sim_k][a, p] > 0), (it, fin, a, p)
            sim_k += 1
        acts = [edt.action(a) for a in _lists(G["act_keys"][it], G["act_lens"][it], n)]
        _, dones = env.perform_action(acts, player=[int(p) for p in current])
        seeds.next = int(G["reset_seed"][it])
        env.reset(env=[i for i, d in enumerate(dones) if d])
    assert sim_k == len(G["sim_step"])


def test_columns_to_deltas_on_host_input():
    """The bitboard -> deltas function of TorchEnv.deltas, fed the harness's simulated columns as CPU tensors."""
    torch = pytest.importorskip("torch")
    ti = importlib.import_module("drl-tetris_amd.torch_interop")
    n, L = 64, 64
    env = _plan_env("harness", n)
    b = env.backend
    player = np.arange(n) % 2
    cnt, lens, keys, pl = _device_lists("harness", b, player, False, L=L)
    cols = _simulate("harness", b, cnt, lens, keys, pl, False, L=L)[0]
    before = b.observe_packed(player=player.astype(np.uint8))[0][0]
    d, s = ti.columns_to_deltas(torch.from_numpy(cols.view(np.int32)), torch.from_numpy(player), torch.from_numpy(before),
                                torch.from_numpy(cnt.get()), 20)
    want_d, want_s = _numpy_deltas(env.get_state(), env.simulate_all_actions(player=player.tolist(), finalize=False), player, L)
    assert d.shape == (n, 20, 10, L) and s.shape == (n, 20, 10, 1)
    assert np.array_equal(d.numpy(), want_d.astype(np.float32))
    assert np.allclose(s.numpy(), want_s, rtol=1e-6, atol=1e-6)
    m = int(cnt.get().max())
    assert np.array_equal(d.numpy()[..., :m], want_d[..., :m].astype(np.float32))      # = the reference's padded array
    assert (d.numpy()[..., m:] == 0).all()


@pytest.mark.gpu
def test_torch_env_deltas():
    torch = pytest.importorskip("torch")
    ti = importlib.import_module("drl-tetris_amd.torch_interop")
    n = 64
    env = _plan_env("hip", n)
    te = ti.TorchEnv(env.backend)
    player = np.arange(n) % 2
    pt = torch.from_numpy(player.astype(np.uint8)).cuda()
    te.action_lists(player=pt)
    d, s = te.deltas(player=pt)
    torch.cuda.synchronize()
    want_d, want_s = _numpy_deltas(env.get_state(), env.simulate_all_actions(player=player.tolist(), finalize=False), player, 64)
    assert np.array_equal(d.cpu().numpy(), want_d.astype(np.float32))
    assert np.allclose(s.cpu().numpy(), want_s, rtol=1e-6, atol=1e-6)
    env.backend.set_stream(None, external=False)


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
@pytest.mark.parametrize("P", [1, 2])
def test_step_lists_matches_step_keys(kind, P):
    n, L, K = _n(kind, 48, 2048), 128, 48
    seeds = orc.episode_seed(np.arange(n), 4)
    a = engines.make(kind, n, P, seeds=seeds)
    r = engines.make(kind, n, P, seeds=seeds)
    rng = np.random.default_rng(10 + P)
    for auto in (False, True):
        for s in range(12):
            player = np.full(n, s % P)
            cnt, lens, keys, pl = _device_lists(kind, a, player, False, L=L, K=K)
            c, ln, kk = cnt.get(), lens.get(), keys.get()
            choice = rng.integers(-3, 60, n).astype(np.int32)             # clamped into [0, count - 1]
            ch = Buf.full(kind, (n,), np.int32)
            ch.put(choice)
            done, lines, dead = Buf.full(kind, (n,), np.uint8), Buf.full(kind, (P, n), np.uint8), Buf.full(kind, (P, n), np.uint8)
            a.step_lists_dev(ch.ptr, cnt.ptr, lens.ptr, keys.ptr, done.ptr, lines.ptr, dead.ptr, max_lists=L, max_keys=K, player=pl.ptr,
                             auto_reset=auto)
            pick = np.clip(choice, 0, c - 1)
            keys_h = np.zeros((n, P, K), np.uint8)
            lens_h = np.ones((n, P), np.uint8)
            keys_h[np.arange(n), player] = kk[np.arange(n), pick]
            lens_h[np.arange(n), player] = ln[np.arange(n), pick]
            d, li, de = r.step_keys(keys_h, lens_h)
            assert np.array_equal(done.get(), d) and np.array_equal(lines.get().T, li) and np.array_equal(dead.get().T, de), (auto, s)
            if auto and d.any():
                m = Buf.full(kind, (n,), np.uint8)
                m.put(d)
                r.reset_dev(m.ptr, None)
            assert np.array_equal(a.snapshot(), r.snapshot()), (auto, s)
    assert a.take_errors() == 0


@pytest.mark.gpu
def test_plan_loop_without_host_sync():
    """200 decisions of lists -> deltas -> choice -> step_lists(auto_reset) at 16 384 two-player games with nothing but
    enqueued work, then the recorded choices replayed through the host path (get_actions + action_list, step_keys, the
    device reset of the finished games) for the first 512 games: same final state."""
    torch = pytest.importorskip("torch")
    ti = importlib.import_module("drl-tetris_amd.torch_interop")
    n, n_check, iters = 16384, 512, 200
    seeds = orc.episode_seed(np.arange(n), 0)
    b = engines.make("hip", n, 2, seeds=seeds)
    te = ti.TorchEnv(b)
    gen = torch.Generator(device="cuda").manual_seed(1234)
    w = torch.rand(n, 20, 10, 1, generator=gen, device="cuda")
    choices, players = [], []
    for it in range(iters):
        pt = torch.full((n,), it % 2, dtype=torch.uint8, device="cuda")
        count, _, _ = te.action_lists(player=pt)
        d, _ = te.deltas(player=pt)
        score = (d * w).sum(dim=(1, 2))
        score = score.masked_fill(torch.arange(score.shape[1], device="cuda")[None, :] >= count[:, None].long(), -1.0)
        choice = score.argmax(dim=1).to(torch.int32)
        te.step_lists(choice, player=pt, auto_reset=True)
        choices.append(choice.clone())
        players.append(it % 2)
    torch.cuda.synchronize()
    assert b.take_errors() == 0
    final = b.snapshot(np.arange(n_check, dtype=np.int32))
    b.set_stream(None, external=False)
    ch = torch.stack(choices).cpu().numpy()
    r = engines.make("hip", n_check, 2, seeds=seeds[:n_check])
    mask = torch.zeros(n_check, dtype=torch.uint8, device="cuda")
    for it in range(iters):
        p = players[it]
        lists = [[list(a) for a in edt.action_list(l, remove_null=True)] for l in r.get_actions(None, np.full(n_check, p))]
        keys = np.zeros((n_check, 2, 48), np.uint8)
        lens = np.ones((n_check, 2), np.uint8)
        for i in range(n_check):
            k = lists[i][int(ch[it, i])]
            keys[i, p, : len(k)] = k
            lens[i, p] = len(k)
        done, _, _ = r.step_keys(keys, lens)
        if done.any():
            mask.copy_(torch.from_numpy(done))
            torch.cuda.synchronize()
            r.reset_dev(mask.data_ptr(), None)
            r.sync()
    assert np.array_equal(r.snapshot(), final)


@pytest.mark.parametrize("kind", engines.ENGINE_PARAMS)
def test_capacity_overflow_is_reported_per_game(kind):
    n = _n(kind, 48, 4096)
    b = engines.make(kind, n, 2, seeds=orc.episode_seed(np.arange(n), 6))
    _scramble(b, 10, 2)
    player = np.zeros(n, np.uint8)
    want = _want_lists(b, player, False)
    some_fit = False
    for L, K in ((4, 8), (24, 8), (40, 6)):
        pad = 64
        cnt = Buf.full(kind, (n + pad,), np.int32, 0x5A5A5A5A)
        lens = Buf.full(kind, (n * L + pad,), np.uint8, 0xAB)
        keys = Buf.full(kind, (n * L * K + pad,), np.uint8, 0xAB)
        pl = Buf.full(kind, (n,), np.uint8)
        pl.put(player)
        b.action_lists_dev(cnt.ptr, lens.ptr, keys.ptr, max_lists=L, max_keys=K, player=pl.ptr)
        c, ln, kk = cnt.get(), lens.get(), keys.get()
        assert (c[n:] == 0x5A5A5A5A).all() and (ln[n * L:] == 0xAB).all() and (kk[n * L * K:] == 0xAB).all(), "wrote past the buffers"
        fits = np.array([len(w) <= L and max(len(x) for x in w) <= K for w in want])
        assert (~fits).any()
        some_fit |= bool(fits.any())
        assert np.array_equal(c[:n] == -1, ~fits), (L, K)
        ln, kk = ln[: n * L].reshape(n, L), kk[: n * L * K].reshape(n, L, K)
        for i in np.nonzero(fits)[0]:
            assert [kk[i, j, : ln[i, j]].tolist() for j in range(c[i])] == want[i]
        for i in np.nonzero(~fits)[0]:
            assert (ln[i] == 0xAB).all() and (kk[i] == 0xAB).all(), "a game that does not fit gets nothing but count -1"
        assert b.take_errors() & ERR_LISTS
        assert b.take_errors() == 0                                      # reported once
    assert some_fit
