"""Zero-copy use of a TetrisBatch from PyTorch-ROCm: actions come from device tensors, observations are written into
device tensors, nothing crosses PCIe.  This is the shape an agent's rollout loop has when its network runs on the same
GPU (worker.py:91-118 with the NN forward pass between get_state and perform_action)."""
import ctypes as C

import numpy as np


def columns_to_deltas(cols, player, before, count, height, out=None, small_fill=1e-3):
    """The deltas of a planning agent from simulated column bitboards (torch tensors, any device):
    cols   int32 [L, P, 10, N]  every player's columns after list k (tetris_simulate_lists_dev without finalize)
    player int64 / uint8 [N]    the acting player of each game
    before uint8 [N, H, W]      the acting player's field > 0 now (observe(player)[0][0])
    count  int32 [N]            lists per game
    -> (deltas float32 [N, H, W, L], sums float32 [N, H, W, 1]).
    Restates sherlock_utils.deltas / generate_deltas (agents/sherlock_agent/sherlock_utils.py:9-20): per list, the acting
    player's field after the list minus the field before; a list whose difference adds up to less than 4 (the piece did not
    land whole, or the player could not move) becomes `small_fill` everywhere; lists past count[i] are zero, which is the
    reference's zero padding to the longest list; sums = the sum over the list axis.  (The reference's state_dict field is
    uint8, and np.full_like on it turns 1e-3 into 0: small_fill=0.0 gives those numbers.)  Fields are occupancy (field > 0)."""
    import torch

    L, P, W, N = cols.shape
    idx = player.to(torch.int64).view(N, 1, 1, 1).expand(N, L, 1, W)
    sel = torch.gather(cols.permute(3, 0, 1, 2), 2, idx).squeeze(2)                       # [N, L, W]
    rows = torch.arange(height, dtype=torch.int32, device=cols.device).view(1, 1, height, 1)
    bits = torch.bitwise_and(torch.bitwise_right_shift(sel.unsqueeze(2), rows), 1)          # [N, L, H, W]
    if out is None:
        out = torch.empty((N, height, W, L), dtype=torch.float32, device=cols.device)
    torch.sub(bits.permute(0, 2, 3, 1), before.unsqueeze(-1), out=out)
    lists = torch.arange(L, device=cols.device).view(1, L)
    small = out.sum(dim=(1, 2)) < 4.0                                                        # [N, L]
    out.masked_fill_(small.view(N, 1, 1, L), small_fill)
    out.masked_fill_((lists >= count.view(N, 1)).view(N, 1, 1, L), 0.0)
    return out, out.sum(dim=-1, keepdim=True)


def kbd_weight_from_conv2d(weight):
    """torch's conv2d kernel [O, C, Hp, 3] (OIHW) -> the keyboard convolution's [Hp, 3, C, O] (HWIO, the reference variable's own
    layout: a checkpoint's kernel needs no transpose), contiguous.  The permute is the same for any kernel size: a residual
    layer's [Co, Ci, 3, 3] becomes its [3, 3, Ci, Co], and kbd_weight_to_conv2d takes it back."""
    return weight.permute(2, 3, 1, 0).contiguous()


def kbd_weight_to_conv2d(weight):
    """[Hp, 3, C, O] (HWIO) -> torch's conv2d kernel [O, C, Hp, 3] (OIHW), contiguous."""
    return weight.permute(3, 2, 0, 1).contiguous()


def keyboard_conv_init(Hp, C, K, device=None, generator=None):
    """The reference's initialisation of keyboard_conv (agents/networks/builders/build_blocks.py:76-77): -> (weight float32
    [Hp, 3, C, 4 K], all zeros; bias float32 [4 K] drawn from a normal distribution of mean 0 and standard deviation 1e-5)."""
    import torch
    weight = torch.zeros(int(Hp), 3, int(C), 4 * int(K), dtype=torch.float32, device=device)
    bias = torch.randn(4 * int(K), dtype=torch.float32, generator=generator) * 1e-5
    return weight, bias.to(device) if device is not None else bias


def residual_layer_init(Ci, Co, device=None, generator=None):
    """The reference's initialisation of a residual layer (agents/networks/builders/build_blocks.py:28, 50): -> (weight float32
    [3, 3, Ci, Co] (HWIO) drawn glorot-uniform, |w| <= sqrt(6 / (fan_in + fan_out)) with fan_in = 9 Ci and fan_out = 9 Co; bias
    float32 [Co], all zeros)."""
    import torch
    limit = (6.0 / (9 * int(Ci) + 9 * int(Co))) ** 0.5
    weight = (torch.rand(3, 3, int(Ci), int(Co), dtype=torch.float32, generator=generator) * 2.0 - 1.0) * limit
    bias = torch.zeros(int(Co), dtype=torch.float32)
    return (weight.to(device), bias.to(device)) if device is not None else (weight, bias)


def pad_channels(x, multiple=8):
    """x [M, C, Hp, 12] -> [M, C', Hp, 12] in channels_last memory, C' = C rounded up to `multiple`, the new channels zero: what
    TorchEnv.residual_layer's rule Ci % 8 == 0 asks of the reference's first layer (1..5 channels from tr.inputs) and of its
    second block's input (128 + len(vector)).  A zero channel stays zero through the ADD join and ELU where it lies at or past Co (the
    join passes it through, and elu(0) = 0) and adds nothing where it lies below; whatever weights face it multiply zeros, so a padded
    trunk computes the unpadded trunk's numbers in the real channels; the rows of the first kernel that face the padding
    get a zero gradient.  x itself when C is a multiple already and its memory is channels_last."""
    import torch
    M, Cn, Hp, Wd = x.shape
    Cp = -(-int(Cn) // int(multiple)) * int(multiple)
    if Cp == Cn and x.is_contiguous(memory_format=torch.channels_last):
        return x
    out = torch.zeros(M, Cp, Hp, Wd, dtype=x.dtype, device=x.device).contiguous(memory_format=torch.channels_last)
    out[:, :Cn] = x
    return out


class TorchEnv:
    def __init__(self, batch, device=None):
        import torch

        self.torch, self.b = torch, batch
        self.dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        n, P, H, W = batch.n_games, batch.n_players, batch.height, batch.width
        u8 = dict(dtype=torch.uint8, device=self.dev)
        self.done = torch.zeros(n, **u8)
        self.lines = torch.zeros(P, n, **u8)          # player-major on the device (tetris_hip.h)
        self.dead = torch.zeros(P, n, **u8)
        self.visual = torch.zeros(P, n, H, W, **u8)
        self.vector = torch.zeros(P, n, 12, **u8)
        self.piece = torch.zeros(P, n, **u8)
        # run the batch on torch's current stream: kernels are ordered with the surrounding torch ops
        batch.set_stream(torch.cuda.current_stream(self.dev).cuda_stream, external=True)

    def _ptr(self, t):
        return None if t is None else C.c_void_p(t.data_ptr())

    def step_rt(self, rot, trans, player=None, ms=400, auto_reset=False):
        """rot/trans/player: uint8 device tensors [n].  -> (done [n], lines [P,n], dead [P,n]) device tensors (reused).
        auto_reset=True: games whose round ended are reset inside the same launch (drl_tetris/worker.py:157-166 without the
        host round trip; seed schedule of include/tetris_hip.h); the outputs describe the step BEFORE the reset.  Nothing in
        this call waits for the GPU: a rollout loop of observe -> policy -> step_rt(auto_reset=True) runs without a host sync."""
        for t in (rot, trans) + (() if player is None else (player,)):
            assert t.dtype == self.torch.uint8 and t.is_cuda and t.is_contiguous() and t.numel() == self.b.n_games
        self.b.step_rt_dev(self._ptr(rot), self._ptr(trans), self._ptr(player), self._ptr(self.done), self._ptr(self.lines),
                           self._ptr(self.dead), ms=ms, auto_reset=auto_reset)
        return self.done, self.lines, self.dead

    def step_rt_observe(self, rot, trans, player=None, next_player=None, ms=400, auto_reset=False):
        """One iteration of the agent loop in one launch: step_rt(...) and observe(next_player) of the stepped state.
        -> (done, lines, dead, visual, vector, piece) device tensors (reused); bit-identical to the two calls."""
        for t in (rot, trans) + tuple(x for x in (player, next_player) if x is not None):
            assert t.dtype == self.torch.uint8 and t.is_cuda and t.is_contiguous() and t.numel() == self.b.n_games
        self.b.step_rt_observe_dev(self._ptr(rot), self._ptr(trans), self._ptr(player), self._ptr(self.done), self._ptr(self.lines),
                                   self._ptr(self.dead), self._ptr(next_player), self._ptr(self.visual), self._ptr(self.vector),
                                   self._ptr(self.piece), ms=ms, auto_reset=auto_reset)
        return self.done, self.lines, self.dead, self.visual, self.vector, self.piece

    def reset(self, mask=None, seeds=None):
        """Device-side reset: mask uint8 [n] device tensor (non-zero = reset; None = all), seeds int16 [n] device tensor
        (None = the built-in schedule).  Only enqueues."""
        if mask is not None:
            assert mask.dtype == self.torch.uint8 and mask.is_cuda and mask.is_contiguous() and mask.numel() == self.b.n_games
        if seeds is not None:
            assert seeds.dtype == self.torch.int16 and seeds.is_cuda and seeds.is_contiguous() and seeds.numel() == self.b.n_games
        self.b.reset_dev(self._ptr(mask), self._ptr(seeds))

    def observe(self, player=None):
        """-> visual [S,n,H,W], vector [S,n,12], piece [S,n] uint8 device tensors; slot 0 = `player`'s own board."""
        self.b._check(self.b.lib.tetris_observe_packed_dev(self.b._h, None, self.b.n_games, self._ptr(player), self._ptr(self.visual),
                                                          self._ptr(self.vector), self._ptr(self.piece)))
        return self.visual, self.vector, self.piece

    # ---- planning on the device: the afterstate loop of a planning agent (agents/sherlock_agent/sherlock_agent.py:94-120)
    def _plan_buffers(self, max_lists, max_keys):
        torch, n, P = self.torch, self.b.n_games, self.b.n_players
        if getattr(self, "_plan_shape", None) == (max_lists, max_keys):
            return
        u8 = dict(dtype=torch.uint8, device=self.dev)
        self._plan_shape = (max_lists, max_keys)
        self.list_count = torch.zeros(n, dtype=torch.int32, device=self.dev)
        self.list_lens = torch.zeros(n, max_lists, **u8)
        self.list_keys = torch.zeros(n, max_lists, max_keys, **u8)
        self.sim_cols = torch.zeros(max_lists, P, 10, n, dtype=torch.int32, device=self.dev)
        self.sim_done = torch.zeros(max_lists, n, **u8)
        self.sim_lines = torch.zeros(max_lists, P, n, **u8)
        self.sim_dead = torch.zeros(max_lists, P, n, **u8)
        self._plan_delta_bufs = {}            # deltas(): (L, dtype, list_major) -> (deltas, sums), allocated on first use
        self.plan_small = torch.zeros(n, max_lists, **u8)

    def _check_player(self, player):
        if player is not None:
            assert player.dtype == self.torch.uint8 and player.is_cuda and player.is_contiguous() and player.numel() == self.b.n_games

    def _lists(self):
        assert getattr(self, "_plan_shape", None) is not None, "call action_lists() first"
        return self._plan_shape

    def action_lists(self, player=None, keep_null=False, max_lists=64, max_keys=48):
        """tetris_environment_vector.get_actions(player) for every game on the device: -> (count int32 [n], lens uint8 [n, L],
        keys uint8 [n, L, K]) device tensors (reused; list k of game i = keys[i, k, :lens[i, k]], count -1 = did not fit:
        take_errors() reports 8).  keep_null: bar_null_moves=False.  player: uint8 device tensor [n] or None (player 0)."""
        self._check_player(player)
        self._plan_buffers(int(max_lists), int(max_keys))
        self.b.action_lists_dev(self._ptr(self.list_count), self._ptr(self.list_lens), self._ptr(self.list_keys), max_lists=max_lists,
                                max_keys=max_keys, player=self._ptr(player), keep_null=keep_null)
        return self.list_count, self.list_lens, self.list_keys

    def simulate(self, player=None, finalize=False, ms=400):
        """simulate_actions of every list of the last action_lists(player) call: -> (cols, done, lines, dead) device tensors
        (reused): cols int32 [L, P, 10, n] = every player's column bitboards (bit y = row y) after list k; with finalize also
        done [L, n], lines / dead [L, P, n].  Entries of lists k >= count[i] are left as they were.  The games are not changed."""
        self._check_player(player)
        L, K = self._lists()
        self.b.simulate_lists_dev(self._ptr(self.list_count), self._ptr(self.list_lens), self._ptr(self.list_keys), self._ptr(self.sim_cols),
                                  max_lists=L, max_keys=K, player=self._ptr(player), finalize=finalize, ms=ms, done=self._ptr(self.sim_done),
                                  lines=self._ptr(self.sim_lines), dead=self._ptr(self.sim_dead))
        return self.sim_cols, self.sim_done, self.sim_lines, self.sim_dead

    def deltas(self, player=None, small_fill=1e-3, dtype=None, list_major=False):
        """sherlock_utils.generate_deltas for every game (lists of the last action_lists(player) call), simulate(finalize=False)
        and one kernel (tetris_plan_deltas_dev): -> (deltas [n, H, W, L], sums [n, H, W, 1]) device tensors, reused per
        (dtype, layout); list_major: deltas [n, L, H, W], sums [n, 1, H, W].  dtype: torch.float32 (default) or torch.float16.
        self.plan_small uint8 [n, L] = 1 where a list fell under the "fewer than 4 cells" rule.  One to four players; values as
        columns_to_deltas, sums by the formula of include/tetris_hip.h."""
        torch = self.torch
        dtype = torch.float32 if dtype is None else dtype
        assert dtype in (torch.float32, torch.float16), "deltas are float32 or float16"
        self._check_player(player)
        cols = self.simulate(player, finalize=False)[0]
        L, _ = self._lists()
        n, H = self.b.n_games, self.b.height
        key = (dtype, bool(list_major))
        bufs = self._plan_delta_bufs
        if key not in bufs:
            shape, sshape = ((n, L, H, 10), (n, 1, H, 10)) if list_major else ((n, H, 10, L), (n, H, 10, 1))
            bufs[key] = (torch.zeros(shape, dtype=dtype, device=self.dev), torch.zeros(sshape, dtype=dtype, device=self.dev))
        d, s = bufs[key]
        self.b.plan_deltas_dev(self._ptr(self.list_count), self._ptr(cols), self._ptr(d), sums=self._ptr(s), small=self._ptr(self.plan_small),
                               max_lists=L, player=self._ptr(player), small_fill=small_fill, f16=dtype == torch.float16, list_major=list_major)
        return d, s

    def step_lists(self, choice, player=None, ms=400, auto_reset=False):
        """perform_action(lists[choice[i]], player) for every game (lists of the last action_lists(player) call); choice: int32
        device tensor [n], clamped into [0, count - 1].  -> (done [n], lines [P, n], dead [P, n]) device tensors (reused).
        auto_reset as for step_rt."""
        assert choice.dtype == self.torch.int32 and choice.is_cuda and choice.is_contiguous() and choice.numel() == self.b.n_games
        self._check_player(player)
        L, K = self._lists()
        self.b.step_lists_dev(self._ptr(choice), self._ptr(self.list_count), self._ptr(self.list_lens), self._ptr(self.list_keys),
                              self._ptr(self.done), self._ptr(self.lines), self._ptr(self.dead), max_lists=L, max_keys=K,
                              player=self._ptr(player), ms=ms, auto_reset=auto_reset)
        return self.done, self.lines, self.dead

    # ---- choosing a list from the network's phi (include/tetris_hip.h: tetris_select_lists_dev, tetris_step_lists_eval_dev): the
    # part of sherlock_agent.get_action between the network and perform_action
    def _plan_eval(self, phi, state_eval, mode, player, seed, draw, small_fill, out_dtype, probs, planes=True):
        """-> (the argument struct, the outputs): the checks, simulate(finalize=False) and the reused output tensors of the two calls"""
        torch, n, H = self.torch, self.b.n_games, self.b.height
        L, _ = self._lists()
        assert L <= 256, "choose_lists takes at most 256 lists per game"
        assert mode in ("argmax", "pi"), "mode is 'argmax' or 'pi'"
        out_dtype = torch.float32 if out_dtype is None else out_dtype
        assert out_dtype in (torch.float32, torch.float16), "delta / sums are float32 or float16"
        for t in (phi,) + (() if state_eval is None else (state_eval,)):
            assert t.dtype in (torch.float32, torch.float16) and t.is_cuda and t.is_contiguous(), "evaluations are contiguous float32 or float16 device tensors"
        assert phi.dim() == 4 and tuple(phi.shape[:3]) == (n, H, 10) and phi.shape[3] in (1, 7), "phi must be [n, H, 10, 7 or 1]"
        if state_eval is not None:
            assert state_eval.dim() == 2 and state_eval.shape[0] == n and state_eval.shape[1] in (1, 7, 8), "state_eval must be [n, 1, 7 or 8]"
        self._check_player(player)
        cols = self.simulate(player, finalize=False)[0]
        if getattr(self, "choose_choice", None) is None:
            f32 = dict(dtype=torch.float32, device=self.dev)
            self.choose_choice = torch.zeros(n, dtype=torch.int32, device=self.dev)
            self.choose_piece = torch.zeros(n, dtype=torch.uint8, device=self.dev)
            self.choose_prob, self.choose_value, self.choose_entropy = torch.zeros(n, **f32), torch.zeros(2, n, **f32), torch.zeros(n, **f32)
            self._choose_planes, self._choose_probs = {}, {}
        if planes and out_dtype not in self._choose_planes:
            self._choose_planes[out_dtype] = tuple(torch.zeros(n, H, 10, dtype=out_dtype, device=self.dev) for _ in range(2))
        delta, sums = self._choose_planes[out_dtype] if planes else (None, None)
        if probs and L not in self._choose_probs:
            self._choose_probs[L] = torch.zeros(n, L, dtype=torch.float32, device=self.dev)
        pr = self._choose_probs[L] if probs else None
        e = self.b.plan_eval(self._ptr(phi), self._ptr(self.list_count), self._ptr(cols), self._ptr(self.choose_choice), n_pieces=phi.shape[3],
                             f16=phi.dtype == torch.float16, state_eval=self._ptr(state_eval),
                             n_values=1 if state_eval is None else state_eval.shape[1],
                             value_f16=state_eval is not None and state_eval.dtype == torch.float16, mode=mode, player=self._ptr(player),
                             seed=seed, draw=draw, small_fill=small_fill, max_lists=L, out_f16=out_dtype == torch.float16,
                             piece=self._ptr(self.choose_piece), prob=self._ptr(self.choose_prob), probs=self._ptr(pr),
                             value=None if state_eval is None else self._ptr(self.choose_value),
                             entropy=self._ptr(self.choose_entropy) if mode == "pi" else None, delta=self._ptr(delta), sums=self._ptr(sums))
        self._choose_last = (e, phi, state_eval, player)             # what Trajectory.record_plan reads (the tensors are kept alive with the struct)
        outs = (self.choose_choice, self.choose_piece, self.choose_prob, None if state_eval is None else self.choose_value,
                self.choose_entropy if mode == "pi" else 0.0, delta, sums) + ((pr,) if probs else ())
        return e, outs

    def choose_lists(self, phi, state_eval=None, mode="argmax", player=None, seed=0, draw=0, small_fill=1e-3, out_dtype=None, probs=False,
                     planes=True):
        """The list of every game (lists of the last action_lists(player) call) from the network's phi [n, H, 10, K] (K = 7, or 1
        with the piece in the state vector; float32 or float16): simulate(finalize=False), then one kernel that scores every list
        with the plane of the piece the game holds, normalises and chooses by mode "argmax" or "pi" (the draw is keyed by (seed,
        global game id, draw): pass the agent's step as `draw`).  The [n, H, 10, L] deltas are never formed.
        -> (choice int32 [n], piece uint8 [n], prob float32 [n] = pi(a), value float32 [2, n] or None, entropy: float32 [n] for
        "pi", else 0.0, delta [n, H, 10] = the chosen list's deltas, sums [n, H, 10] = the sum over the lists; out_dtype:
        torch.float32 (default) or torch.float16) and with probs=True also probs float32 [n, L] — device tensors, reused; choice
        feeds step_lists unchanged.  The games are not changed; nothing waits for the GPU.  planes=False: delta and sums are not
        asked of the kernel and None stands in their place — the form for an actor whose window keeps the packed record
        (Trajectory(plan=True).record_plan)."""
        e, outs = self._plan_eval(phi, state_eval, mode, player, seed, draw, small_fill, out_dtype, probs, planes)
        self.b.select_lists_dev(e)
        return outs

    def step_lists_eval(self, phi, state_eval=None, mode="argmax", player=None, seed=0, draw=0, small_fill=1e-3, out_dtype=None, probs=False,
                        ms=400, auto_reset=False, planes=True):
        """choose_lists + step_lists in one call: -> (done [n], lines [P, n], dead [P, n]) + choose_lists' outputs; auto_reset as
        for step_rt."""
        e, outs = self._plan_eval(phi, state_eval, mode, player, seed, draw, small_fill, out_dtype, probs, planes)
        _, K = self._lists()
        self.b.step_lists_eval_dev(e, self._ptr(self.list_lens), self._ptr(self.list_keys), self._ptr(self.done), self._ptr(self.lines),
                                   self._ptr(self.dead), max_keys=K, ms=ms, auto_reset=auto_reset)
        return (self.done, self.lines, self.dead) + outs

    # ---- heuristic policy on the device (include/tetris_hip.h: tetris_rt_features_dev and the four after it)
    def _policy_buffers(self):
        if getattr(self, "policy_rot", None) is not None:
            return
        torch, n = self.torch, self.b.n_games
        self.policy_rot = torch.zeros(n, dtype=torch.uint8, device=self.dev)
        self.policy_trans = torch.zeros(n, dtype=torch.uint8, device=self.dev)
        self.policy_score = torch.zeros(n, dtype=torch.int32, device=self.dev)

    def _check_weights(self, weights):
        """weights: int16 device tensor [8] (one vector for the batch) or [n, 8] (one per game) -> per_game"""
        assert weights.dtype == self.torch.int16 and weights.is_cuda and weights.is_contiguous()
        assert tuple(weights.shape) in ((8,), (self.b.n_games, 8)), "weights must be [8] or [n, 8]"
        return weights.dim() == 2

    def rt_features(self, player=None):
        """The eight POLICY_FEATURE_NAMES features of the 40 (r, t) candidate fields of every game (candidate c = 10 r + t):
        -> int16 [40, 8, n] device tensor (reused).  The games are not changed."""
        self._check_player(player)
        if getattr(self, "policy_features", None) is None:
            self.policy_features = self.torch.zeros(40, 8, self.b.n_games, dtype=self.torch.int16, device=self.dev)
        self.b.rt_features_dev(self._ptr(self.policy_features), player=self._ptr(player))
        return self.policy_features

    def policy_rt(self, weights, player=None):
        """The best-scoring candidate of every game (score = weights . features, lowest 10 r + t among equals):
        -> (rot uint8 [n], trans uint8 [n], score int32 [n]) device tensors (reused); rot / trans feed step_rt unchanged."""
        self._check_player(player)
        per_game = self._check_weights(weights)
        self._policy_buffers()
        self.b.policy_rt_dev(self._ptr(weights), self._ptr(self.policy_rot), self._ptr(self.policy_trans), self._ptr(self.policy_score),
                             player=self._ptr(player), per_game=per_game)
        return self.policy_rot, self.policy_trans, self.policy_score

    def step_policy(self, weights, player=None, ms=400, auto_reset=False):
        """policy_rt + step_rt in one call (the scripted opponent's move): -> (done [n], lines [P, n], dead [P, n], rot [n],
        trans [n]) device tensors (reused); auto_reset as for step_rt."""
        self._check_player(player)
        per_game = self._check_weights(weights)
        self._policy_buffers()
        self.b.step_policy_dev(self._ptr(weights), self._ptr(self.done), self._ptr(self.lines), self._ptr(self.dead),
                               rot=self._ptr(self.policy_rot), trans=self._ptr(self.policy_trans), player=self._ptr(player),
                               per_game=per_game, ms=ms, auto_reset=auto_reset)
        return self.done, self.lines, self.dead, self.policy_rot, self.policy_trans

    def game_totals(self):
        """The built-in rollouts' per-game counters: -> int32 [4, n] device tensor (reused; the words are uint32): env-steps,
        episodes, lines cleared, garbage lines sent of every game — a population's fitness without a host loop."""
        if getattr(self, "policy_totals", None) is None:
            self.policy_totals = self.torch.zeros(4, self.b.n_games, dtype=self.torch.int32, device=self.dev)
        self.b.rollout_game_totals_dev(self._ptr(self.policy_totals))
        return self.policy_totals

    # ---- acting on a network's (r, t, piece) evaluation (include/tetris_hip.h: tetris_select_eval_dev and the two after it):
    # the part of sventon_agent.get_action between the network and perform_action
    def _act_eval(self, action_eval, state_eval, mode, player, seed, draw, epsilon, theta, table):
        """-> (the argument struct, value or None, entropy): the checks and the reused output tensors of the three calls"""
        from . import capi
        torch, n = self.torch, self.b.n_games
        for t in (action_eval,) + (() if state_eval is None else (state_eval,)):
            assert t.dtype in (torch.float32, torch.float16) and t.is_cuda and t.is_contiguous(), "evaluations are contiguous float32 or float16 device tensors"
        assert action_eval.dim() == 4 and tuple(action_eval.shape[:3]) == (n, 4, 10) and action_eval.shape[3] in (1, 7), "action_eval must be [n, 4, 10, 7 or 1]"
        if state_eval is not None:
            assert state_eval.dim() == 2 and state_eval.shape[0] == n and state_eval.shape[1] in (1, 7, 8), "state_eval must be [n, 1, 7 or 8]"
        self._check_player(player)
        if getattr(self, "act_rot", None) is None:
            u8, f32 = dict(dtype=torch.uint8, device=self.dev), dict(dtype=torch.float32, device=self.dev)
            self.act_rot, self.act_trans, self.act_piece = torch.zeros(n, **u8), torch.zeros(n, **u8), torch.zeros(n, **u8)
            self.act_chosen, self.act_value, self.act_entropy = torch.zeros(n, **f32), torch.zeros(2, n, **f32), torch.zeros(n, **f32)
        if mode == "rank":
            assert (theta is None) != (table is None), "the rank mode takes theta or a table"
            table = capi.pareto_table(theta) if table is None else np.ascontiguousarray(table, dtype=np.float32)
        else:
            table = None
        e = self.b.act_eval(self._ptr(action_eval), self._ptr(self.act_rot), self._ptr(self.act_trans), n_pieces=action_eval.shape[3],
                            f16=action_eval.dtype == torch.float16, state_eval=self._ptr(state_eval),
                            n_values=1 if state_eval is None else state_eval.shape[1],
                            value_f16=state_eval is not None and state_eval.dtype == torch.float16, mode=mode, player=self._ptr(player),
                            seed=seed, draw=draw, epsilon=epsilon, table=table, piece=self._ptr(self.act_piece), eval=self._ptr(self.act_chosen),
                            value=None if state_eval is None else self._ptr(self.act_value), entropy=self._ptr(self.act_entropy) if mode == "pi" else None)
        entropy = self.act_entropy if mode == "pi" else capi.act_entropy(mode, epsilon, table)
        self._act_last = (e, player, state_eval)         # what Trajectory.record reads (the tensors are kept alive with the struct)
        return e, (None if state_eval is None else self.act_value), entropy

    def select_eval(self, action_eval, state_eval=None, mode="argmax", player=None, seed=0, draw=0, epsilon=0.0, theta=None, table=None):
        """The (r, t) of every game from the network's action_eval [n, 4, 10, K] (K = 7, or 1 with the piece in the state vector;
        float32 or float16): the map of the piece the game holds, then mode "argmax", "pi" (the map as a distribution), "rank" (the
        reference's pareto: theta, or a table of 40 weights by rank) or "epsilon".  The draw is keyed by (seed, global game id,
        draw): pass the agent's step as `draw`.  state_eval [n, V] (V = 1, 7, 8) gives value = (v(s | piece), mean v(s)).
        -> (rot [n], trans [n], piece [n] uint8, eval float32 [n] = the chosen entry, value float32 [2, n] or None, entropy:
        float32 [n] for "pi", else the reference's number as a Python float) — device tensors, reused; rot / trans feed step_rt
        unchanged.  The games are not changed; nothing waits for the GPU."""
        e, value, entropy = self._act_eval(action_eval, state_eval, mode, player, seed, draw, epsilon, theta, table)
        self.b.select_eval_dev(e)
        return self.act_rot, self.act_trans, self.act_piece, self.act_chosen, value, entropy

    def step_eval(self, action_eval, state_eval=None, mode="argmax", player=None, seed=0, draw=0, epsilon=0.0, theta=None, table=None,
                  ms=400, auto_reset=False):
        """select_eval + step_rt in one call: -> (done [n], lines [P, n], dead [P, n]) + select_eval's outputs; auto_reset as for
        step_rt."""
        e, value, entropy = self._act_eval(action_eval, state_eval, mode, player, seed, draw, epsilon, theta, table)
        self.b.step_eval_dev(e, self._ptr(self.done), self._ptr(self.lines), self._ptr(self.dead), ms=ms, auto_reset=auto_reset)
        return self.done, self.lines, self.dead, self.act_rot, self.act_trans, self.act_piece, self.act_chosen, value, entropy

    def step_eval_observe(self, action_eval, state_eval=None, mode="argmax", player=None, next_player=None, seed=0, draw=0, epsilon=0.0,
                          theta=None, table=None, ms=400, auto_reset=False):
        """step_eval and observe(next_player) of the stepped state (one or two players): -> (done, lines, dead, visual, vector,
        piece [S, n] of the observation) + select_eval's outputs.  The agent loop is network forward, this call, network forward."""
        self._check_player(next_player)
        e, value, entropy = self._act_eval(action_eval, state_eval, mode, player, seed, draw, epsilon, theta, table)
        self.b.step_eval_observe_dev(e, self._ptr(self.done), self._ptr(self.lines), self._ptr(self.dead), self._ptr(next_player),
                                     self._ptr(self.visual), self._ptr(self.vector), self._ptr(self.piece), ms=ms, auto_reset=auto_reset)
        return (self.done, self.lines, self.dead, self.visual, self.vector, self.piece, self.act_rot, self.act_trans, self.act_piece,
                self.act_chosen, value, entropy)

    # ---- trajectory windows (include/tetris_hip.h: tetris_traj_record_dev, tetris_traj_advantages_dev): the worker-side arithmetic
    # between perform_action and the data packet (drl_tetris/worker.py:103-112)
    def trajectory(self, capacity, states=False, plan=False):
        """A window of `capacity` rows of this batch's games: -> Trajectory (device tensors, allocated once).  states: the window
        also holds the packed observation records (observe / select / batch).  plan (needs states): it also holds the planning
        agent's packed delta records (record_plan / batch_plan)."""
        return Trajectory(self, capacity, states, plan)

    # ---- experience replay (include/tetris_hip.h: tetris_replay_add_dev and the three after it): the buffer of
    # sventon_agent_dqn_trainer.do_training (agents/sventon_agent/sventon_agent_dqn_trainer.py:30-100)
    def replay(self, capacity, k_step=1, seed=0):
        """A prioritised replay of `capacity` entries (the reference's max_size argument) with k-step views: -> Replay (device
        tensors, allocated once).  seed: the key of the sampling draws."""
        return Replay(self, capacity, k_step, seed)

    # ---- loss heads (include/tetris_hip.h: tetris_ppo_loss_dev, tetris_dqn_loss_dev): the arithmetic of the two trainers'
    # create_training_ops between the network's outputs and the optimiser (agents/networks/ppo_nets.py:141-196, prio_qnet.py:102-117)
    def _loss_inputs(self, x, action, per_sample, valid):
        """the checks both heads share -> M"""
        torch = self.torch
        assert x.dtype in (torch.float32, torch.float16) and x.is_cuda and x.is_contiguous(), "the evaluation is a contiguous float32 or float16 device tensor"
        assert x.dim() == 4 and tuple(x.shape[1:3]) == (4, 10) and x.shape[3] in (1, 7), "the evaluation must be [M, 4, 10, 7 or 1]"
        M = x.shape[0]
        assert action.dtype == torch.uint8 and action.is_cuda and action.is_contiguous() and tuple(action.shape) == (M, 3), "action must be uint8 [M, 3]"
        for t in per_sample:
            assert t.dtype == torch.float32 and t.is_cuda and t.is_contiguous() and t.numel() == M, "per-sample inputs are contiguous float32 [M]"
        if valid is not None:
            assert valid.dtype == torch.uint8 and valid.is_cuda and valid.is_contiguous() and valid.numel() == M, "valid must be uint8 [M]"
        return M

    def _loss_buffers(self, key, M, make):
        """One set of output tensors per head, piece count and element type, made for `capacity` samples by make(capacity): a
        larger M replaces the set by one of that size (the old one is dropped), a smaller M uses its leading part."""
        if getattr(self, "_loss_cache", None) is None:
            self._loss_cache = {}
        have = self._loss_cache.get(key)
        if have is None or have[0] < M:
            have = self._loss_cache[key] = (max(M, 1), make(max(M, 1)))
        return have[1]

    def ppo_head(self, pi, v, action, prob_old, adv, target, valid=None, *, clipping_parameter, value_loss, policy_loss, entropy_loss,
                 ppo_epsilon, entropy_floor_loss, rescaled_entropy, grad_scale=1.0, terms=False):
        """The PPO loss of a minibatch from the network's pi [M, 4, 10, K] and v [M, V] (K = 7 or 1, V = 1 or K; float32 or
        float16): create_training_ops' loss, statistics and the gradient of the loss with respect to pi and v, scaled by grad_scale
        (an AMP loss scale).  action uint8 [M, 3], prob_old / adv / target float32 [M] and valid uint8 [M] are the fields of
        Trajectory.batch(...) as they come; the parameter names are model.train's, all required (entropy_floor_loss = 0 /
        rescaled_entropy = 0 stand for the reference's params without that key; ppo_epsilon gives the entropy floor).
        -> (stats float32 [16] in the order of capi.PPO_STATS, grad_pi like pi, grad_v like v[, terms float32 [6, M] in the order of
        capi.PPO_TERMS]) — device tensors, reused by every call with the same K, V and element type (the leading M samples of one
        set that grows to the largest M seen); nothing waits for the GPU."""
        torch = self.torch
        M = self._loss_inputs(pi, action, (prob_old, adv, target), valid)
        assert v.dtype in (torch.float32, torch.float16) and v.is_cuda and v.is_contiguous(), "v is a contiguous float32 or float16 device tensor"
        K = pi.shape[3]
        assert v.dim() == 2 and v.shape[0] == M and v.shape[1] in (1, K), "v must be [M, 1 or K]"
        V = v.shape[1]

        def make(cap):
            f32 = dict(dtype=torch.float32, device=self.dev)
            return (torch.zeros(16, **f32), torch.zeros(cap, 4, 10, K, dtype=pi.dtype, device=self.dev),
                    torch.zeros(cap, V, dtype=pi.dtype, device=self.dev), torch.zeros(6 * cap, **f32))
        stats, grad_pi, grad_v, t = self._loss_buffers(("ppo", K, V, pi.dtype), M, make)
        grad_pi, grad_v, t = grad_pi[:M], grad_v[:M], t[:6 * M].view(6, M)
        p = self._ptr
        l = self.b.ppo_loss(p(pi), p(v), p(action), p(prob_old), p(adv), p(target), p(grad_pi), p(grad_v), p(stats), M, n_pieces=K, n_values=V,
                            valid=p(valid), terms=p(t) if terms else None, f16=pi.dtype == torch.float16, value_f16=v.dtype == torch.float16,
                            grad_f16=pi.dtype == torch.float16, clipping_parameter=clipping_parameter, value_loss=value_loss,
                            policy_loss=policy_loss, entropy_loss=entropy_loss, ppo_epsilon=ppo_epsilon, entropy_floor_loss=entropy_floor_loss,
                            rescaled_entropy=rescaled_entropy, grad_scale=grad_scale)
        self.b.ppo_loss_dev(l)
        return (stats, grad_pi, grad_v, t) if terms else (stats, grad_pi, grad_v)

    def dqn_head(self, Q, action, target, weight=None, valid=None, optimistic_prios=0.0, grad_scale=1.0):
        """The DQN loss of a minibatch from the network's Q [M, 4, 10, K] (float32 or float16): the importance-weighted mean squared
        error of Q[r, t, piece] against target (weight float32 [M] = Replay.sample's, or None), its statistics, its gradient with
        respect to Q scaled by grad_scale, and the samples' new priorities |q - target| (+ optimistic_prios relu of it).
        -> (stats float32 [16] in the order of capi.DQN_STATS, grad_Q like Q, new_prio float32 [M], q float32 [M]) — device tensors,
        reused as ppo_head's are; new_prio is what Replay.update_prios(index, new_prio) takes."""
        torch = self.torch
        M = self._loss_inputs(Q, action, (target,) + (() if weight is None else (weight,)), valid)
        K = Q.shape[3]

        def make(cap):
            f32 = dict(dtype=torch.float32, device=self.dev)
            return torch.zeros(16, **f32), torch.zeros(cap, 4, 10, K, dtype=Q.dtype, device=self.dev), torch.zeros(cap, **f32), torch.zeros(cap, **f32)
        stats, grad_Q, new_prio, q = self._loss_buffers(("dqn", K, Q.dtype), M, make)
        grad_Q, new_prio, q = grad_Q[:M], new_prio[:M], q[:M]
        p = self._ptr
        l = self.b.dqn_loss(p(Q), p(action), p(target), p(grad_Q), p(new_prio), p(stats), M, n_pieces=K, weight=p(weight), valid=p(valid), q=p(q),
                            f16=Q.dtype == torch.float16, grad_f16=Q.dtype == torch.float16, optimistic_prios=optimistic_prios,
                            grad_scale=grad_scale)
        self.b.dqn_loss_dev(l)
        return stats, grad_Q, new_prio, q

    def plan_head(self, phi, v, traj, index, piece, prob_old, adv, target, valid=None, *, small_fill, clipping_parameter, value_loss,
                  policy_loss, entropy_loss, impossibility_loss, grad_scale=1.0, terms=False):
        """The planning agent's PPO loss (delta_ppo_nets.create_training_ops) of a minibatch from the network's RAW phi [M, H, 10, K]
        (the head clips) and v [M, V] (K = 7 or 1, V = 1 or K; float32 or float16) and the plan records of traj =
        Trajectory(plan=True): index int32 [M] as for traj.batch / batch_plan (bit 31: mirrored; an index that names no entry is an
        invalid sample), piece uint8 [M] — mb.action[:, 2] of traj.batch(index) serves as it is, a view with a stride of 3 bytes —,
        prob_old / adv / target float32 [M] and valid uint8 [M] as Trajectory.batch gives them.  delta and delta_sum are never
        expanded; small_fill has batch_plan's meaning (0.0: the reference's numbers).  The parameter names are model.train's, all
        required.  -> (stats float32 [16] in the order of capi.PLAN_LOSS_STATS, grad_phi like phi, grad_v like v[, terms float32
        [6, M] in the order of capi.PLAN_LOSS_TERMS]) — device tensors, reused as ppo_head's are; nothing waits for the GPU."""
        torch = self.torch
        H = self.b.height
        assert hasattr(traj, "plan_rec"), "the window was made without plan=True"
        assert phi.dtype in (torch.float32, torch.float16) and phi.is_cuda and phi.is_contiguous(), "phi is a contiguous float32 or float16 device tensor"
        assert phi.dim() == 4 and tuple(phi.shape[1:3]) == (H, 10) and phi.shape[3] in (1, 7), "phi must be [M, H, 10, 7 or 1]"
        M, K = phi.shape[0], phi.shape[3]
        assert v.dtype in (torch.float32, torch.float16) and v.is_cuda and v.is_contiguous(), "v is a contiguous float32 or float16 device tensor"
        assert v.dim() == 2 and v.shape[0] == M and v.shape[1] in (1, K), "v must be [M, 1 or K]"
        V = v.shape[1]
        assert index.dtype == torch.int32 and index.is_cuda and index.is_contiguous() and index.numel() == M, "index must be int32 [M]"
        assert piece.dtype == torch.uint8 and piece.is_cuda and piece.dim() == 1 and piece.numel() == M, "piece must be uint8 [M]"
        stride = piece.stride(0) if M > 1 else 1
        assert stride >= 1, "piece must not be a broadcast view"
        for t in (prob_old, adv, target):
            assert t.dtype == torch.float32 and t.is_cuda and t.is_contiguous() and t.numel() == M, "per-sample inputs are contiguous float32 [M]"
        if valid is not None:
            assert valid.dtype == torch.uint8 and valid.is_cuda and valid.is_contiguous() and valid.numel() == M, "valid must be uint8 [M]"

        def make(cap):
            f32 = dict(dtype=torch.float32, device=self.dev)
            return (torch.zeros(16, **f32), torch.zeros(cap, H, 10, K, dtype=phi.dtype, device=self.dev),
                    torch.zeros(cap, V, dtype=phi.dtype, device=self.dev), torch.zeros(6 * cap, **f32))
        stats, grad_phi, grad_v, t = self._loss_buffers(("plan", K, V, phi.dtype), M, make)
        grad_phi, grad_v, t = grad_phi[:M], grad_v[:M], t[:6 * M].view(6, M)
        p = self._ptr
        l = self.b.plan_loss(p(phi), p(v), p(index), p(piece), p(prob_old), p(adv), p(target), p(grad_phi), p(grad_v), p(stats), M, n_pieces=K,
                             n_values=V, piece_stride=stride, valid=p(valid), terms=p(t) if terms else None, f16=phi.dtype == torch.float16,
                             value_f16=v.dtype == torch.float16, grad_f16=phi.dtype == torch.float16, small_fill=small_fill,
                             clipping_parameter=clipping_parameter, value_loss=value_loss, policy_loss=policy_loss, entropy_loss=entropy_loss,
                             impossibility_loss=impossibility_loss, grad_scale=grad_scale)
        self.b.plan_loss_dev(traj._plan, l)
        return (stats, grad_phi, grad_v, t) if terms else (stats, grad_phi, grad_v)

    def _head_function(self):
        """the torch.autograd.Function of both losses: forward runs a head and keeps its gradients, backward hands them on"""
        torch = self.torch
        if getattr(self, "_head_fn", None) is None:
            class HeadLoss(torch.autograd.Function):
                @staticmethod
                def forward(ctx, run, *outputs_of_the_network):
                    loss, grads, others = run()
                    ctx.grads = [g if g.dtype == x.dtype else g.to(x.dtype) for g, x in zip(grads, outputs_of_the_network)]
                    ctx.mark_non_differentiable(*others)
                    return (loss,) + tuple(others)

                @staticmethod
                def backward(ctx, grad_loss, *unused):
                    return (None,) + tuple(g * grad_loss.to(g.dtype) for g in ctx.grads)
            self._head_fn = HeadLoss
        return self._head_fn

    def ppo_loss(self, pi, v, action, prob_old, adv, target, valid=None, **params):
        """ppo_head as a differentiable loss: -> (loss, stats) with loss a 0-dim float32 tensor (stats[1], copied) whose backward()
        hands grad_pi and grad_v, times the incoming gradient, to pi and v — te.ppo_loss(*net(mb.visual, mb.vector), mb.action,
        mb.prob, mb.adv, mb.target, mb.valid, clipping_parameter=..., ...)[0].backward(); opt.step().  The gradients are ppo_head's
        reused tensors, not copies: call backward before the next ppo_loss of the same shape.  With grad_scale = s the gradients
        are s times those of the returned loss (the optimiser's unscale undoes it)."""
        def run():
            stats, grad_pi, grad_v = self.ppo_head(pi.detach(), v.detach(), action, prob_old, adv, target, valid, **params)[:3]
            return stats[1].clone(), (grad_pi, grad_v), (stats,)
        return self._head_function().apply(run, pi, v)

    def plan_loss(self, phi, v, traj, index, piece, prob_old, adv, target, valid=None, **params):
        """plan_head as a differentiable loss: -> (loss, stats) with loss a 0-dim float32 tensor (stats[1], copied) whose backward()
        hands grad_phi and grad_v, times the incoming gradient, to phi and v:
            idx = index[perm[:M]]; mb = tr.batch(idx); v, phi = net(mb.visual, mb.vector)
            loss, stats = te.plan_loss(phi, v, tr, idx, mb.action[:, 2], mb.prob, mb.adv, mb.target, mb.valid, small_fill=0.0, ...)
            loss.backward(); opt.step()
        As for ppo_loss the gradients are plan_head's reused tensors: call backward before the next plan_loss of the same shape."""
        def run():
            stats, grad_phi, grad_v = self.plan_head(phi.detach(), v.detach(), traj, index, piece, prob_old, adv, target, valid, **params)[:3]
            return stats[1].clone(), (grad_phi, grad_v), (stats,)
        return self._head_function().apply(run, phi, v)

    def dqn_loss(self, Q, action, target, weight=None, valid=None, optimistic_prios=0.0, grad_scale=1.0):
        """dqn_head as a differentiable loss: -> (loss, stats, new_prio) with loss a 0-dim float32 tensor (stats[2], copied) whose
        backward() hands grad_Q, times the incoming gradient, to Q; then rp.update_prios(index, new_prio).  As for ppo_loss the
        gradient is dqn_head's reused tensor."""
        def run():
            stats, grad_Q, new_prio, _ = self.dqn_head(Q.detach(), action, target, weight, valid, optimistic_prios, grad_scale)
            return stats[2].clone(), (grad_Q,), (stats, new_prio)
        return self._head_function().apply(run, Q)

    # ---- output heads (include/tetris_hip.h: tetris_q_head_dev, tetris_policy_head_dev and their _grad_dev): from a trunk's raw
    # streams to Q / V / A (network_utils.qva_from_raw_streams) and to pi / v (ppo_nets.py:24-33), differentiable
    def _head_streams(self, big, small, widths, what):
        """the checks both heads share -> (M, K, width of `small` or 0)"""
        torch = self.torch
        assert big.dtype in (torch.float32, torch.float16) and big.is_cuda, f"{what[0]} is a float32 or float16 device tensor"
        assert big.dim() == 4 and tuple(big.shape[1:3]) == (4, 10) and big.shape[3] in (1, 7) and big.shape[0] >= 1, f"{what[0]} must be [M, 4, 10, 7 or 1]"
        M, K = int(big.shape[0]), int(big.shape[3])
        if small is None:
            return M, K, 0
        assert small.dtype in (torch.float32, torch.float16) and small.is_cuda, f"{what[1]} is a float32 or float16 device tensor"
        assert small.dim() == 2 and small.shape[0] == M and small.shape[1] in widths(K), f"{what[1]} must be [M, {' or '.join(str(w) for w in widths(K))}]"
        return M, K, int(small.shape[1])

    def _head_functions(self):
        """the two torch.autograd.Functions: forward runs a head into the reused output tensors, backward its _grad entry point"""
        torch = self.torch
        if getattr(self, "_head_fns", None) is not None:
            return self._head_fns
        env, p = self, self._ptr

        class QHead(torch.autograd.Function):
            @staticmethod
            def forward(ctx, a, v, cfg):
                a, v = a.detach().contiguous(), None if v is None else v.detach().contiguous()
                M, K, Kv = env._head_streams(a, v, lambda K: (1, K), ("a", "v"))
                vdt = a.dtype if v is None else v.dtype

                def make(cap):
                    big = lambda: torch.zeros(cap, 4, 10, K, dtype=a.dtype, device=env.dev)                      # noqa: E731
                    return big(), torch.zeros(cap, dtype=torch.float32, device=env.dev), big(), big(), torch.zeros(cap, max(Kv, 1), dtype=vdt, device=env.dev)
                Q, V, A, grad_a, grad_v = (t[:M] for t in env._loss_buffers(("q_head", K, Kv, a.dtype, vdt), M, make))
                kw = dict(n_pieces=K, n_values=max(Kv, 1), mode=cfg["mode"], advantage_range=cfg["advantage_range"],
                          separate_piece_values=cfg["separate_piece_values"], used_pieces=cfg["pieces"], f16=a.dtype == torch.float16,
                          value_f16=vdt == torch.float16)
                env.b.q_head_dev(env.b.q_head(p(a), M, v=p(v), Q=p(Q), V=p(V), A=p(A) if cfg["A"] else None, **kw))
                ctx.a, ctx.v, ctx.kw, ctx.grads = a, v, kw, (grad_a, grad_v)
                ctx.mark_non_differentiable(V, A)
                return Q, V, A

            @staticmethod
            def backward(ctx, grad_Q, *unused):
                a, v, (grad_a, grad_v) = ctx.a, ctx.v, ctx.grads
                grad_Q = (torch.zeros_like(a) if grad_Q is None else grad_Q.to(a.dtype)).contiguous()
                env.b.q_head_grad_dev(env.b.q_head(p(a), a.shape[0], v=p(v), grad_Q=p(grad_Q), grad_a=p(grad_a),
                                                   grad_v=None if v is None else p(grad_v), **ctx.kw))
                return grad_a, None if v is None else grad_v, None

        class PolicyHead(torch.autograd.Function):
            @staticmethod
            def forward(ctx, x, w):
                x, w = x.detach().contiguous(), w.detach().contiguous()
                M, K, W = env._head_streams(x, w, lambda K: (1, K + 1), ("x", "w"))
                V = 1 if W == 1 else K

                def make(cap):
                    big = lambda: torch.zeros(cap, 4, 10, K, dtype=x.dtype, device=env.dev)                      # noqa: E731
                    return big(), torch.zeros(cap, V, dtype=w.dtype, device=env.dev), big(), torch.zeros(cap, W, dtype=w.dtype, device=env.dev)
                pi, v, grad_x, grad_w = (t[:M] for t in env._loss_buffers(("policy_head", K, W, x.dtype, w.dtype), M, make))
                kw = dict(n_pieces=K, n_values=W, f16=x.dtype == torch.float16, value_f16=w.dtype == torch.float16)
                env.b.policy_head_dev(env.b.policy_head(M, p(pi), p(v), x=p(x), w=p(w), **kw))
                ctx.out, ctx.kw, ctx.grads = (pi, v), kw, (grad_x, grad_w)
                return pi, v

            @staticmethod
            def backward(ctx, grad_pi, grad_v):
                (pi, v), (grad_x, grad_w) = ctx.out, ctx.grads
                grad_pi = (torch.zeros_like(pi) if grad_pi is None else grad_pi.to(pi.dtype)).contiguous()
                grad_v = (torch.zeros_like(v) if grad_v is None else grad_v.to(v.dtype)).contiguous()
                env.b.policy_head_grad_dev(env.b.policy_head(pi.shape[0], p(pi), p(v), grad_pi=p(grad_pi), grad_v=p(grad_v), grad_x=p(grad_x),
                                                             grad_w=p(grad_w), **ctx.kw))
                return grad_x, grad_w
        self._head_fns = (QHead, PolicyHead)
        return self._head_fns

    def q_head(self, a, v=None, mode="mean", advantage_range=1.0, separate_piece_values=True, pieces=None, A=False):
        """The DQN nets' output head (qva_from_raw_streams as base_architecture.py:53-62 calls it) from a trunk's raw streams: a =
        _A [M, 4, 10, K] and v = _V [M, 1 or K] or None (prio_qnet's full_network=False: 0), float32 or float16, K = 7 or 1.
        mode "mean" / "max" / anything else (no normalisation), advantage_range and separate_piece_values are the reference's
        settings; pieces = the used-piece mask (bit p), None: the batch's piece set.  -> (Q like a, V float32 [M][, A like a with
        A=True]), differentiable through Q with respect to a and v; V and A carry no gradient (the trainers differentiate Q only).
            te.select_eval(te.q_head(*qnet(visual, vector))[0], ...); te.dqn_loss(te.q_head(*qnet(mb.visual, mb.vector))[0], ...)
        Device tensors, reused by every call with the same K, width of v and element types (the leading M samples of one set that
        grows to the largest M seen): use Q — select, loss, targets — before the next q_head of the same shapes; backward needs only
        a and v, which it recomputes from.  Nothing waits for the GPU."""
        cfg = dict(mode=mode, advantage_range=float(advantage_range), separate_piece_values=bool(separate_piece_values),
                   pieces=self.b.used_pieces(a.shape[3]) if pieces is None else int(pieces), A=bool(A))
        Q, V, A_out = self._head_functions()[0].apply(a, v, cfg)
        return (Q, V, A_out) if A else (Q, V)

    def policy_head(self, x, w):
        """The PPO nets' output head (ppo_nets.py:24-33) from a trunk's raw streams: x = the logits [M, 4, 10, K] as keyboard_conv's
        concat lays them out, w = the value stream [M, 1 or K + 1], float32 or float16.  -> (pi like x: action_softmax over the 40
        (r, t) of each piece; v [M, 1 or K] like w: tanh of w_0 plus the mean-free piece values), the shapes ppo_loss takes:
            te.ppo_loss(*te.policy_head(*net(mb.visual, mb.vector)), mb.action, mb.prob, mb.adv, mb.target, mb.valid, ...)
        Differentiable with respect to x and w.  Device tensors, reused as q_head's are; backward reads the stored pi and v: call it
        before the next policy_head of the same shapes.  Nothing waits for the GPU."""
        return self._head_functions()[1].apply(x, w)

    # ---- keyboard convolution (include/tetris_hip.h: tetris_kbd_conv_dev and its _grad_x_dev / _grad_w_dev): the network's last
    # learned layer (agents/networks/builders/build_blocks.py:68-83), differentiable
    def _kbd_input(self, x):
        """x [M, C, Hp, 12] as the library reads it: itself when its memory is channels_last (NHWC), else one layout copy"""
        torch = self.torch
        return x if x.is_contiguous(memory_format=torch.channels_last) else x.contiguous(memory_format=torch.channels_last)

    def _kbd_function(self):
        torch = self.torch
        if getattr(self, "_kbd_fn", None) is not None:
            return self._kbd_fn
        env, p = self, self._ptr

        class KeyboardConv(torch.autograd.Function):
            @staticmethod
            def forward(ctx, x, weight, bias):
                assert x.dtype in (torch.float32, torch.float16) and x.is_cuda, "x is a float32 or float16 device tensor"
                assert x.dim() == 4 and x.shape[3] == 12 and x.shape[0] >= 1, "x must be [M, C, Hp, 12]"
                M, Cn, Hp = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
                assert weight.dim() == 4 and tuple(weight.shape[:3]) == (Hp, 3, Cn) and weight.shape[3] % 4 == 0, "weight must be [Hp, 3, C, 4 K]"
                K = int(weight.shape[3]) // 4
                assert bias.dtype == torch.float32 and tuple(bias.shape) == (4 * K,) and bias.is_cuda, "bias is a float32 device tensor [4 K]"
                xl = env._kbd_input(x.detach())
                w = weight.detach().to(x.dtype).contiguous()
                b32 = bias.detach().contiguous()

                def make(cap):
                    return (torch.zeros(cap, 4, 10, K, dtype=x.dtype, device=env.dev),
                            torch.zeros(cap, Cn, Hp, 12, dtype=x.dtype, device=env.dev).contiguous(memory_format=torch.channels_last),
                            torch.zeros(Hp, 3, Cn, 4 * K, dtype=torch.float32, device=env.dev), torch.zeros(4 * K, dtype=torch.float32, device=env.dev))
                out, grad_x, grad_w, grad_b = env._loss_buffers(("kbd_conv", Hp, Cn, K, x.dtype), M, make)
                kw = dict(m=M, height=Hp, channels=Cn, n_pieces=K, f16=x.dtype == torch.float16)
                env.b.kbd_conv_dev(env.b.kbd_conv(x=p(xl), w=p(w), bias=p(b32), out=p(out), **kw))
                ctx.x, ctx.w, ctx.kw, ctx.grads, ctx.types = xl, w, kw, (grad_x[:M], grad_w, grad_b), (weight.dtype, bias.dtype)
                return out[:M]

            @staticmethod
            def backward(ctx, grad_out):
                (grad_x, grad_w, grad_b), (wdt, bdt) = ctx.grads, ctx.types
                g = grad_out.to(ctx.x.dtype).contiguous()
                need_x, need_w, need_b = ctx.needs_input_grad
                if need_x:
                    env.b.kbd_conv_grad_x_dev(env.b.kbd_conv(w=p(ctx.w), grad_out=p(g), grad_x=p(grad_x), **ctx.kw))
                if need_w or need_b:
                    env.b.kbd_conv_grad_w_dev(env.b.kbd_conv(x=p(ctx.x), grad_out=p(g), grad_w=p(grad_w), grad_b=p(grad_b), **ctx.kw))
                return (grad_x if need_x else None, grad_w.to(wdt) if need_w else None, grad_b.to(bdt) if need_b else None)
        self._kbd_fn = KeyboardConv
        return self._kbd_fn

    def keyboard_conv(self, x, weight, bias):
        """The reference's keyboard_conv (agents/networks/builders/build_blocks.py:68-83, without its activation, which q_head and
        policy_head apply): a "valid" convolution of the trunk's output x [M, C, Hp, 12] with a kernel as tall as the image and three
        columns wide, and the four channel slices concatenated along the rotation axis, on the matrix cores.  x float32 or
        float16, C a multiple of 32 in 32..512, Hp in 4..33; weight [Hp, 3, C, 4 K] (HWIO: kbd_weight_from_conv2d gives it from a
        conv2d kernel), cast to x's type when it is a float32 master weight; bias float32 [4 K], K in 1..7.  -> [M, 4, 10, K] in
        x's type, differentiable with respect to x, weight and bias (grad_w and grad_b in the parameters' types):
            out = te.select_eval(te.q_head(te.keyboard_conv(trunk(visual, vector), w, b))[0], mode="argmax")
        x is read in place when its memory is channels_last (tr.inputs(channels_last=True) and a channels_last trunk give that);
        otherwise it is COPIED once with .contiguous(memory_format=torch.channels_last), forward and for grad_w.  Device tensors,
        reused by every call with the same Hp, C, K and element type (the leading M samples of one set that grows to the largest M
        seen): use the output — heads, select, loss — and call backward before the next keyboard_conv of the same shapes; the
        gradients handed back are reused likewise.  Nothing waits for the GPU."""
        return self._kbd_function().apply(x, weight, bias)

    # ---- residual layer (include/tetris_hip.h: tetris_res_layer_dev and its _grad_x_dev / _grad_w_dev): one layer of the trunk's
    # residual_block (agents/networks/builders/build_blocks.py:8-64), differentiable
    def _res_function(self):
        torch = self.torch
        if getattr(self, "_res_fn", None) is not None:
            return self._res_fn
        from . import capi
        env, p = self, self._ptr

        class ResidualLayer(torch.autograd.Function):
            @staticmethod
            def forward(ctx, x, weight, bias, join, activation, slot):
                assert x.dtype in (torch.float32, torch.float16) and x.is_cuda, "x is a float32 or float16 device tensor"
                assert x.dim() == 4 and x.shape[3] == 12 and x.shape[0] >= 1, "x must be [M, Ci, Hp, 12]"
                M, Ci, Hp = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
                assert weight.dim() == 4 and tuple(weight.shape[:3]) == (3, 3, Ci), "weight must be [3, 3, Ci, Co]"
                Co = int(weight.shape[3])
                assert bias.dtype == torch.float32 and tuple(bias.shape) == (Co,) and bias.is_cuda, "bias is a float32 device tensor [Co]"
                Cout = capi.res_out_channels(Ci, Co, join)
                xl = env._kbd_input(x.detach())
                w = weight.detach().to(x.dtype).contiguous()
                b32 = bias.detach().contiguous()

                def make(cap):
                    last = lambda c: torch.zeros(cap, c, Hp, 12, dtype=x.dtype, device=env.dev).contiguous(memory_format=torch.channels_last)      # noqa: E731
                    return (last(Cout), last(Ci), torch.zeros(3, 3, Ci, Co, dtype=torch.float32, device=env.dev), torch.zeros(Co, dtype=torch.float32, device=env.dev))
                base = ("res_layer", Hp, Ci, Co, join, activation, x.dtype)
                ctx.pending = None
                if slot is None:
                    # a set of its own for every forward of these shapes whose backward is still to come (they end in the
                    # reverse order, so the count is a stack), and never the set whose output this layer reads
                    pending = env._res_pending.get(base, 0)
                    out = env._loss_buffers(base + (("auto", pending),), M, make)[0]
                    index = pending + 1 if out.data_ptr() == xl.data_ptr() else pending
                    slot = ("auto", index)
                    if any(ctx.needs_input_grad[:3]):
                        ctx.pending = base
                        env._res_pending[base] = index + 1
                out, grad_x, grad_w, grad_b = env._loss_buffers(base + (slot,), M, make)
                kw = dict(m=M, height=Hp, in_channels=Ci, out_channels=Co, join=join, activation=activation, f16=x.dtype == torch.float16)
                env.b.res_layer_dev(env.b.res_layer(x=p(xl), w=p(w), bias=p(b32), out=p(out), **kw))
                ctx.x, ctx.w, ctx.y, ctx.kw, ctx.grads, ctx.types = xl, w, out, kw, (grad_x[:M], grad_w, grad_b), (weight.dtype, bias.dtype)
                return out[:M]

            @staticmethod
            def backward(ctx, grad_out):
                (grad_x, grad_w, grad_b), (wdt, bdt) = ctx.grads, ctx.types
                g = grad_out.to(ctx.x.dtype).contiguous(memory_format=torch.channels_last)
                need_x, need_w, need_b = ctx.needs_input_grad[:3]
                if ctx.pending is not None:
                    env._res_pending[ctx.pending] = max(env._res_pending.get(ctx.pending, 0) - 1, 0)
                    ctx.pending = None
                if need_x:
                    env.b.res_layer_grad_x_dev(env.b.res_layer(w=p(ctx.w), y=p(ctx.y), grad_out=p(g), grad_x=p(grad_x), **ctx.kw))
                if need_w or need_b:
                    env.b.res_layer_grad_w_dev(env.b.res_layer(x=p(ctx.x), y=p(ctx.y), grad_out=p(g), grad_w=p(grad_w), grad_b=p(grad_b), **ctx.kw))
                return (grad_x if need_x else None, grad_w.to(wdt) if need_w else None, grad_b.to(bdt) if need_b else None, None, None, None)
        self._res_fn, self._res_pending = ResidualLayer, {}
        return self._res_fn

    def residual_release(self):
        """Forget the forwards of residual_layer whose backward never came (a graph that was dropped): their buffer sets are
        handed out again."""
        if getattr(self, "_res_pending", None) is not None:
            self._res_pending.clear()

    def residual_layer(self, x, weight, bias, join="add", activation="elu", slot=None):
        """One layer of the reference's residual_block (agents/networks/builders/build_blocks.py:43-57): conv2d(3 x 3, 'same'),
        peephole_join(mode=join) (agents/networks/network_utils.py:52-64), activation, fused on the matrix cores.  x [M, Ci, Hp, 12]
        float32 or float16, Ci a multiple of 8 in 8..512 (pad_channels gives that), Hp in 4..33; weight [3, 3, Ci, Co] (HWIO:
        kbd_weight_from_conv2d gives it from a conv2d kernel, residual_layer_init draws it), Co a multiple of 32 in 32..512, cast to
        x's type when it is a float32 master weight; bias float32 [Co]; join "add" / "truncate_add" / None; activation "elu" / None.
        -> a channels_last tensor [M, Cout, Hp, 12] in x's type, Cout = max(Ci, Co) / min(Ci, Co) / Co, differentiable with respect
        to x, weight and bias (grad_w and grad_b in the parameters' types).  x is read in place when its memory is channels_last
        (tr.inputs(channels_last=True), pad_channels and this function's own output give that), so layers chain without copies and
        the last one feeds keyboard_conv without one; otherwise it is COPIED once.  Device tensors, reused per shape, settings and
        element type (the leading M samples of one set that grows to the largest M seen).  Backward reads each layer's stored
        input and output, so layers whose shapes agree must not share a set: with slot=None (the default) a forward that
        needs a gradient takes a set of its own until its backward has run — the sets are counted per shape, and the same ones
        come round in the next step —, and a forward without one alternates between two sets so that a chain never writes what
        it reads.  A graph that is dropped without backward keeps its sets until residual_release().  slot=<any hashable> names
        the set instead; then the caller keeps layers of equal shape apart.  Nothing waits for the GPU."""
        from . import capi
        assert join in capi.RES_JOINS and activation in capi.RES_ACTS, "join is 'add', 'truncate_add' or None; activation 'elu' or None"
        return self._res_function().apply(x, weight, bias, join or "none", activation or "none", slot)

    def residual_block(self, x, params, output_activation="elu", output_n_filters=None, slot=None):
        """The reference's residual_block with its defaults (peepholes=True, no pools, no dropout, no normalisation): params is a
        list of (weight [3, 3, Ci, Co], bias [Co]), one per layer; every layer is ADD + ELU, the last one takes output_activation
        and, when output_n_filters is given (it must be the last weight's Co), TRUNCATE_ADD.  -> [M, Cout, Hp, 12], channels_last.
        slot=None: every layer finds its own buffer set (residual_layer); slot=k: the layers take the sets k, k + 1, ..."""
        n = len(params)
        for i, (weight, bias) in enumerate(params):
            last = i == n - 1
            join = "truncate_add" if last and output_n_filters is not None else "add"
            if last and output_n_filters is not None:
                assert int(weight.shape[3]) == int(output_n_filters), "the last layer's Co is output_n_filters"
            x = self.residual_layer(x, weight, bias, join=join, activation=output_activation if last else "elu",
                                    slot=None if slot is None else slot + i)
        return x

    # ---- k-step target estimator (include/tetris_hip.h: tetris_kstep_target_dev): model.compute_targets
    # (agents/sventon_agent/sventon_agent_dqn_trainer.py:49-59, agents/networks/value_estimator.py:51-88)
    def _kstep(self, cache, out, reward, done, index, max_size, k_step, steps, gamma, lam, truncate, used_pieces, values):
        """the checks and the call both modes share -> target float32 [M], reused per M in `cache`"""
        from . import capi
        torch = self.torch
        steps = capi.kstep_steps(k_step) if steps is None else [int(s) for s in steps]
        n = len(steps)
        assert n >= 1, "no step"
        assert out.dtype in (torch.float32, torch.float16) and out.is_cuda and out.is_contiguous(), "the net's output is a contiguous float32 or float16 device tensor"
        if values:
            assert out.dim() == 2 and out.shape[1] in (1, 7), "v must be [M * n, 7 or 1]"
            K = V = int(out.shape[1])
        else:
            assert out.dim() == 4 and tuple(out.shape[1:3]) == (4, 10) and out.shape[3] in (1, 7), "Q must be [M * n, 4, 10, 7 or 1]"
            K, V = int(out.shape[3]), 1
        assert out.shape[0] % n == 0, "the net's output has a row per (sample, step)"
        M = out.shape[0] // n
        for t, dt in ((reward, torch.float32), (done, torch.uint8)):
            assert t.dtype == dt and t.is_cuda and t.is_contiguous()
        if index is None:
            assert reward.numel() == M * (k_step + 1) and done.numel() == M * (k_step + 1), "reward / done must be [M, k_step + 1]"
        else:
            assert index.dtype == torch.int32 and index.is_cuda and index.is_contiguous() and index.numel() == M
        if M not in cache:
            cache[M] = torch.zeros(max(M, 1), dtype=torch.float32, device=self.dev)
        target = cache[M]
        p = self._ptr
        t = self.b.kstep_target(p(out), p(reward), p(done), p(target), M, k_step, steps=steps, index=p(index), max_size=max_size,
                                values_mode=values, n_pieces=K, n_values=V, used_pieces=used_pieces, f16=out.dtype == torch.float16,
                                truncate=truncate, gamma=gamma, lam=lam)
        self.b.kstep_target_dev(t)
        return target[:M]

    def kstep_targets(self, out, reward, done, steps=None, k_step=None, gamma=0.99, lam=0.9, truncate=False, used_pieces=None, values=False):
        """The k-step targets of M samples in array mode, for callers without a ring: out = Q [M * n, 4, 10, K] (values=True: v
        [M * n, V]) float32 or float16, the net's output for the n steps of `steps` (None: 1..k_step) of every sample, sample-major;
        reward float32 / done uint8 [M, k_step + 1], the samples' rows 0..k_step (k_step None: from reward's shape).  -> float32
        [M], reused per M.  No host synchronisation."""
        k = int(reward.shape[1]) - 1 if k_step is None else int(k_step)
        if not hasattr(self, "_kstep_targets"):
            self._kstep_targets = {}
        return self._kstep(self._kstep_targets, out, reward, done, None, 0, k, steps, gamma, lam, truncate, used_pieces, values)


    # ---- network inputs (include/tetris_hip.h: tetris_net_input_dev): the cast, apply_visual_pad and visual_stack
    # (agents/networks/network_utils.py:71-93) of a network's first layer, straight from packed observation records
    def _net_input(self, cache, key, lead, source, items, pad, dtype, channels_last):
        """the checks and the call the three wrappers share: `lead` = the sample dimensions ([M] or [M, steps]); source = the
        keywords of capi's net_input that name the records -> (visual, vector, piece, valid), reused per (key, lead, settings)"""
        from . import capi
        torch = self.torch
        assert dtype in (torch.float32, torch.float16), "the inputs are float32 or float16"
        items = tuple(items)
        assert len(items) <= 4 and len(set(items)) == len(items) and all(i in capi.INPUT_ITEMS for i in items), \
            f"items: up to four distinct names of {tuple(capi.INPUT_ITEMS)}"
        S = self.b.n_players
        Cn, Hp, Wp = capi.input_shape(self.b.height, len(items), pad)
        full = (key, tuple(lead), items, bool(pad), dtype, bool(channels_last))
        if full not in cache:
            f, u8 = dict(dtype=dtype, device=self.dev), dict(dtype=torch.uint8, device=self.dev)
            k = len(lead)
            if channels_last:          # the memory of a torch channels_last tensor, handed out in the logical (channels-first) shape
                visual = torch.zeros(S, *lead, Hp, Wp, Cn, **f).permute(*range(1 + k), 3 + k, 1 + k, 2 + k)
            else:
                visual = torch.zeros(S, *lead, Cn, Hp, Wp, **f)
            cache[full] = (visual, torch.zeros(S, *lead, 12, **f), torch.zeros(S, *lead, **u8), torch.zeros(*lead, **u8))
        out = cache[full]
        visual, vector, piece, valid = out
        if visual.numel() == 0:
            return out
        p = self._ptr
        self.b.net_input_dev(self.b.net_input(items=items, pad=pad, f16=dtype == torch.float16, channels_last=channels_last, visual=p(visual),
                                              vector=p(vector), piece=p(piece), valid=p(valid), **source))
        return out

    def net_input(self, player=None, items=("cumsum", "shadow", "height", "holes"), pad=True, dtype=None, channels_last=False):
        """The network's input of the games' current state for an actor without a window, perspective of player (uint8 [n] or None:
        player 0): the records of tetris_traj_observe_dev into a private one-row buffer, then their padded plane stacks — two
        launches, no uint8 planes in between.  -> (visual [S, n, C, Hp, Wp], vector [S, n, 12], piece uint8 [S, n], valid uint8 [n]),
        as Trajectory.inputs(row=...) gives them; reused device tensors, nothing waits for the GPU.  One and two players."""
        torch, n = self.torch, self.b.n_games
        self._check_player(player)
        if getattr(self, "_input_obs", None) is None:
            assert self.b.n_players <= 2, "the packed observation is defined for one or two players"
            self._input_rec = torch.zeros(1, n, self.b.n_players, 12, dtype=torch.int32, device=self.dev)
            self._input_obs, self._inputs = self.b.traj_obs(1, self._ptr(self._input_rec)), {}
        self.b.traj_observe_dev(self._input_obs, 0, self._ptr(player))
        return self._net_input(self._inputs, "row", (n,), dict(m=n, obs=self._input_obs, row=0), items, pad,
                               torch.float32 if dtype is None else dtype, channels_last)


class Trajectory:
    """A trajectory window of a TorchEnv: T = capacity rows of n games, time-major device tensors
        action uint8 [T, n, 4] (r, t, piece, acting player), prob float32 [T, n] (the chosen entry), value float32 [2, T, n]
        (v(s | piece), mean v(s)), reward float32 [T, n], done uint8 [T, n].
    record(row) replaces store_experience, advantages(...) sventon_trajectory.process_trajectory(compute_advantages=True)
    (agents/datatypes/trajectory.py:56-86, 111-141).  The actor loop is network forward, step_eval_observe, record, and every T
    steps one advantages call; everything is reused device tensors and nothing waits for the GPU.  A caller with rewards of
    their own (dual-policy re-pairing, extra rewards) fills `reward` / `done` themselves and calls advantages.
    With states=True the window also holds obs int32 [T, n, S, 12] (the words are uint32), the packed observation record of
    include/tetris_hip.h: observe(row) before the acting call of the row, then after advantages select(...) lists the finished
    entries and batch(index) expands a minibatch of them, mirrored or not, into the trainer's arrays.
    With plan=True (a planning agent: sherlock_trajectory, sherlock_agent_ppo_trainer.do_training) the window also holds plan_rec
    int32 [T, n, 112] (the words are uint32), the plan record of include/tetris_hip.h — 448 bytes per entry in place of two float
    [H, 10] planes.  The loop is observe(row), action_lists, step_lists_eval(planes=False), record_plan(row); advantages, select
    and batch serve unchanged (action[:, 0] is the list's index, action[:, 1] carries no meaning), and batch_plan(index) expands
    delta(s, a) and delta_sum(s) of the same samples."""

    def __init__(self, env, capacity, states=False, plan=False):
        torch, n = env.torch, env.b.n_games
        assert int(capacity) >= 1, "a window has at least one row"
        self.env, self.capacity = env, int(capacity)
        u8, f32 = dict(dtype=torch.uint8, device=env.dev), dict(dtype=torch.float32, device=env.dev)
        T = self.capacity
        self.action, self.prob, self.value = torch.zeros(T, n, 4, **u8), torch.zeros(T, n, **f32), torch.zeros(2, T, n, **f32)
        self.reward, self.done = torch.zeros(T, n, **f32), torch.zeros(T, n, **u8)
        self.adv, self.target, self.closed = torch.zeros(T, n, **f32), torch.zeros(T, n, **f32), torch.zeros(T, n, **u8)
        p = env._ptr
        self._traj = env.b.traj(T, p(self.action), p(self.prob), p(self.value), p(self.reward), p(self.done))
        if states:
            assert env.b.n_players <= 2, "the packed observation is defined for one or two players"
            self.obs = torch.zeros(T, n, env.b.n_players, 12, dtype=torch.int32, device=env.dev)
            self._obs = env.b.traj_obs(T, p(self.obs))
            self.count = torch.zeros(1, dtype=torch.int32, device=env.dev)
            self._index, self._batches, self._rows = {}, {}, 0
        assert states or not plan, "plan=True requires states=True (the record's `before` is the observation's)"
        if plan:
            from . import capi
            self.plan_rec = torch.zeros(T, n, capi.PLAN_REC_WORDS, dtype=torch.int32, device=env.dev)
            self._plan = env.b.traj_plan(T, p(self.plan_rec))
            self._plan_batches = {}

    def record_plan(self, row):
        """Row `row` from the last choose_lists / step_lists_eval call of the TorchEnv (with or without planes) and the step's done /
        dead: the list's index, piece, pi(a), values and player into the row arrays as record does, and the plan record from the
        lists' simulated columns and the row's observation — call observe(row) before action_lists of the row.  One and two
        players."""
        env = self.env
        assert hasattr(self, "plan_rec"), "the window was made without plan=True"
        last = getattr(env, "_choose_last", None)
        assert last is not None, "call choose_lists or step_lists_eval first"
        env.b.traj_record_plan_dev(self._traj, self._plan, self._obs, row, last[0], env._ptr(env.done), env._ptr(env.dead))

    def batch_plan(self, index, small_fill=1e-3, dtype=None):
        """delta(s, a) and delta_sum(s) of the samples index names (as for batch; bit 31: the mirrored image, which the reference
        does not have) -> TrajectoryPlanBatch(delta [M, H, 10, 1], sums [M, H, 10, 1]) device tensors, reused per (M, dtype); dtype:
        torch.float32 (default) or torch.float16.  small_fill=0.0 gives the reference's numbers."""
        from collections import namedtuple
        env, torch = self.env, self.env.torch
        assert hasattr(self, "plan_rec"), "the window was made without plan=True"
        assert index.dtype == torch.int32 and index.is_cuda and index.is_contiguous() and index.dim() == 1
        dtype = torch.float32 if dtype is None else dtype
        assert dtype in (torch.float32, torch.float16), "delta / sums are float32 or float16"
        M, H = index.numel(), env.b.height
        if (M, dtype) not in self._plan_batches:
            kind = namedtuple("TrajectoryPlanBatch", "delta sums")
            self._plan_batches[(M, dtype)] = kind(*(torch.zeros(M, H, 10, 1, dtype=dtype, device=env.dev) for _ in range(2)))
        t = self._plan_batches[(M, dtype)]
        if M == 0:
            return t
        env.b.traj_plan_batch_dev(self._plan, env._ptr(index), M, delta=env._ptr(t.delta), sums=env._ptr(t.sums), small_fill=small_fill,
                                  f16=dtype == torch.float16)
        return t

    def record(self, row):
        """Row `row` from the last step_eval / step_eval_observe call of the TorchEnv: its (r, t, piece), chosen entry, values
        (zeros without a state_eval) and player, the step's done, and the reference's reward (tetris_environment.reward_fcn
        without extra_rewards) from done / dead.  One and two players."""
        env = self.env
        last = getattr(env, "_act_last", None)
        assert last is not None, "call step_eval or step_eval_observe first"
        env.b.traj_record_dev(self._traj, row, last[0], env._ptr(env.done), env._ptr(env.dead))

    def advantages(self, rows, gamma, gae_lambda, gve_lambda=0.95, bootstrap=None):
        """adv_and_targets over rows 0 .. rows-1, every episode of every game separately: -> (adv float32 [rows, n], target float32
        [rows, n], closed uint8 [rows, n]) views of reused device tensors.  closed = 1: the entry's episode ended inside the
        window and adv / target are the reference's numbers; the open tail is cut off with bootstrap float32 [n] = the value[0]
        the next row would have (None: zero).  gamma may be negative (single-policy self-play)."""
        env, torch = self.env, self.env.torch
        if bootstrap is not None:
            assert bootstrap.dtype == torch.float32 and bootstrap.is_cuda and bootstrap.is_contiguous() and bootstrap.numel() == env.b.n_games
        p = env._ptr
        env.b.traj_advantages_dev(self._traj, rows, gamma, gae_lambda, gve_lambda, p(bootstrap), p(self.adv), p(self.target), p(self.closed))
        if hasattr(self, "obs"):
            self._rows = rows
        return self.adv[:rows], self.target[:rows], self.closed[:rows]

    # ---- states and sample sets (include/tetris_hip.h: tetris_traj_observe_dev, tetris_traj_select_dev, tetris_traj_batch_dev)
    def observe(self, row, player=None):
        """Row `row` of obs from the games' current state, perspective of player (uint8 [n] or None: player 0): call it before the
        acting call of the row — observe(row), step_eval_observe, record(row)."""
        assert hasattr(self, "obs"), "the window was made without states=True"
        self.env._check_player(player)
        self.env.b.traj_observe_dev(self._obs, row, self.env._ptr(player))

    def select(self, rows, mask=None, augment=False, capacity=None):
        """The flat indices t n + i of the non-zero entries of mask uint8 [rows, n] (None: closed of the last advantages call) in
        ascending order, with augment followed by the same list with bit 31 set (augment_data's concatenation): -> (index int32
        [capacity], count int32 [1]) device tensors, reused; -1 past the list; count is the full length even when it exceeds
        capacity (default: rows n, twice that with augment)."""
        env, torch = self.env, self.env.torch
        assert hasattr(self, "obs"), "the window was made without states=True"
        n = env.b.n_games
        if mask is None:
            assert 1 <= rows <= self._rows, "no advantages call covers these rows"
            mask = self.closed
        assert mask.dtype == torch.uint8 and mask.is_cuda and mask.is_contiguous() and mask.numel() >= rows * n
        cap = rows * n * (2 if augment else 1) if capacity is None else int(capacity)
        if cap not in self._index:
            self._index[cap] = torch.zeros(max(cap, 1), dtype=torch.int32, device=env.dev)
        index = self._index[cap]
        env.b.traj_select_dev(env._ptr(mask), rows, env._ptr(index), cap, env._ptr(self.count), augment=augment)
        return index[:cap], self.count

    def batch(self, index):
        """The samples index (int32 device tensor [M]: a slice of select's list, permuted at will; bit 31 = mirrored, -1 = none)
        names -> TrajectoryBatch(visual [S, M, H, 10], vector [S, M, 12], piece [S, M], action [M, 3], prob, adv, target, reward
        [M], done, valid [M]) device tensors, reused per M.  adv / target are those of the last advantages call."""
        from collections import namedtuple
        env, torch = self.env, self.env.torch
        assert hasattr(self, "obs"), "the window was made without states=True"
        assert index.dtype == torch.int32 and index.is_cuda and index.is_contiguous() and index.dim() == 1
        M, S, H = index.numel(), env.b.n_players, env.b.height
        if M not in self._batches:
            u8, f32 = dict(dtype=torch.uint8, device=env.dev), dict(dtype=torch.float32, device=env.dev)
            kind = namedtuple("TrajectoryBatch", "visual vector piece action prob adv target reward done valid")
            t = kind(torch.zeros(S, M, H, 10, **u8), torch.zeros(S, M, 12, **u8), torch.zeros(S, M, **u8), torch.zeros(M, 3, **u8),
                     torch.zeros(M, **f32), torch.zeros(M, **f32), torch.zeros(M, **f32), torch.zeros(M, **f32), torch.zeros(M, **u8),
                     torch.zeros(M, **u8))
            self._batches[M] = (t, env.b.traj_batch(*[env._ptr(x) for x in t]))
        t, out = self._batches[M]
        env.b.traj_batch_dev(self._traj, self._obs, env._ptr(index), M, out, adv=env._ptr(self.adv), target=env._ptr(self.target))
        return t

    def inputs(self, index=None, row=None, items=("cumsum", "shadow", "height", "holes"), pad=True, dtype=None, channels_last=False):
        """The network's first-layer inputs of a set of the window's entries straight from their packed records (tetris_net_input_dev:
        the cast to float, apply_visual_pad and visual_stack of agents/networks/network_utils.py:71-93; batch's uint8 planes are
        never written): index as for batch (int32 device tensor [M]; bit 31 = mirrored, -1 = none), or row = a row of the window in
        game order, M = n — the actor's form: observe(row), then inputs(row=row).  items: the reference's `items` list, in channel
        order, () for the plain float planes; pad=False: the legacy encoder's pad_visuals=False; dtype torch.float32 (default) or
        torch.float16.  -> (visual [S, M, C, Hp, Wp], vector [S, M, 12] of dtype, piece uint8 [S, M], valid uint8 [M]) device tensors,
        reused per shape and settings; C = 1 + len(items), Hp = H + 2 and Wp = 12 with pad.  channels_last=True: the same logical
        shape as a permuted view of [S, M, Hp, Wp, C], so visual[s] is a torch channels_last tensor (the reference's NHWC)."""
        env, torch = self.env, self.env.torch
        assert hasattr(self, "obs"), "the window was made without states=True"
        assert (index is None) != (row is None), "either an index list or a row"
        if not hasattr(self, "_inputs"):
            self._inputs = {}
        dtype = torch.float32 if dtype is None else dtype
        if index is None:
            assert 0 <= int(row) < self.capacity, "row outside the window"
            n = env.b.n_games
            return env._net_input(self._inputs, "row", (n,), dict(m=n, obs=self._obs, row=int(row)), items, pad, dtype, channels_last)
        assert index.dtype == torch.int32 and index.is_cuda and index.is_contiguous() and index.dim() == 1
        M = index.numel()
        return env._net_input(self._inputs, "index", (M,), dict(m=M, obs=self._obs, index=env._ptr(index)), items, pad, dtype, channels_last)


class Replay:
    """The prioritised experience replay of a TorchEnv (agents/agent_utils/experience_replay.py in its rank mode), on the device:
    capacity C entries of which max_size = C - k_step take samples, as device tensors
        obs int32 [C, S, 12] (the packed observation record), action uint8 [C, 4], prob / adv / target / reward float32 [C],
        done / flags uint8 [C] (flags bit 0: the mirrored sample), prio float32 [max_size], cursor int32 [4] (current_idx,
        current_size, samples offered so far, entries dropped).
    add(tr, rows) takes the finished entries of a Trajectory(states=True) window, sample(M, alpha, beta, draw) the reference's
    get_random_sample, gather(index, steps) the k-step views as the trainer's arrays, update_prios(index, prio) the new
    priorities.  Nothing waits for the GPU but len() and dropped(), which read the cursor."""

    def __init__(self, env, capacity, k_step=1, seed=0):
        torch = env.torch
        C_, k = int(capacity), int(k_step)
        assert k >= 0 and 1 <= C_ - k <= 1 << 24, "k_step >= 0 and 1 <= capacity - k_step <= 2^24"
        assert env.b.n_players <= 2, "the packed observation is defined for one or two players"
        self.env, self.capacity, self.k_step, self.max_size, self.seed = env, C_, k, C_ - k, int(seed)
        u8, f32, i32 = (dict(dtype=d, device=env.dev) for d in (torch.uint8, torch.float32, torch.int32))
        self.obs, self.action = torch.zeros(C_, env.b.n_players, 12, **i32), torch.zeros(C_, 4, **u8)
        self.prob, self.adv, self.target, self.reward = (torch.zeros(C_, **f32) for _ in range(4))
        self.done, self.flags = torch.zeros(C_, **u8), torch.zeros(C_, **u8)
        self.prio, self.cursor = torch.zeros(self.max_size, **f32), torch.zeros(4, **i32)
        self.count = torch.zeros(1, **i32)
        p = env._ptr
        self._rp = env.b.replay(C_, k, p(self.obs), p(self.action), p(self.prob), p(self.adv), p(self.target), p(self.reward), p(self.done),
                                p(self.flags), p(self.prio), p(self.cursor))
        self._samples, self._batches = {}, {}

    def add(self, tr, rows, mask=None, augment=True, prio=None):
        """The entries of mask uint8 [rows, n] (None: closed of the window's last advantages call) of the window tr, game-major,
        with its adv / target; augment: every game's run once more as the mirrored samples; prio float32 [rows, n] (None: 2.0,
        the reference's "very large prio")."""
        env, torch = self.env, self.env.torch
        assert hasattr(tr, "obs"), "the window was made without states=True"
        n = env.b.n_games
        if mask is None:
            assert 1 <= rows <= tr._rows, "no advantages call covers these rows"
            mask = tr.closed
        assert mask.dtype == torch.uint8 and mask.is_cuda and mask.is_contiguous() and mask.numel() >= rows * n
        if prio is not None:
            assert prio.dtype == torch.float32 and prio.is_cuda and prio.is_contiguous() and prio.numel() >= rows * n
        p = env._ptr
        env.b.replay_add_dev(self._rp, tr._traj, tr._obs, p(mask), rows, adv=p(tr.adv), target=p(tr.target), prio=p(prio), augment=augment)

    def sample(self, M, alpha, beta, draw=0, rank=False):
        """get_random_sample(M, alpha, beta) in rank mode: -> (index int32 [M], weight float32 [M], count int32 [1]) device tensors,
        reused per M: the min(M, len) entries drawn without replacement, -1 / 0 past them.  The draw is keyed by (seed, position,
        draw): pass the update's number as `draw`.  rank=True: also self.rank int32 [max_size] and self.key float32 [max_size]."""
        env, torch = self.env, self.env.torch
        M = int(M)
        if M not in self._samples:
            self._samples[M] = (torch.zeros(max(M, 1), dtype=torch.int32, device=env.dev), torch.zeros(max(M, 1), dtype=torch.float32, device=env.dev))
        index, weight = self._samples[M]
        if rank and getattr(self, "rank", None) is None:
            self.rank = torch.zeros(self.max_size, dtype=torch.int32, device=env.dev)
            self.key = torch.zeros(self.max_size, dtype=torch.float32, device=env.dev)
        p = env._ptr
        env.b.replay_sample_dev(self._rp, M, alpha, beta, self.seed, draw, p(index), p(weight), p(self.count),
                                rank=p(self.rank) if rank else None, key=p(self.key) if rank else None)
        return index[:M], weight[:M], self.count

    def gather(self, index, steps=1):
        """The k-step views of index (int32 device tensor [M]; -1: none) -> TrajectoryBatch(visual [S, M, steps, H, 10], vector [S,
        M, steps, 12], piece [S, M, steps], action [M, steps, 3], prob, adv, target, reward, done, valid [M, steps]) device tensors,
        reused per (M, steps); 1 <= steps <= k_step + 1.  steps may also be a sequence of step numbers within [0, k_step]
        (capi.kstep_steps: the rows the target estimator's net is evaluated on): the same arrays with len(steps) in the place of
        steps, in ascending order of the step, reused per (M, tuple of the steps)."""
        from collections import namedtuple
        env, torch = self.env, self.env.torch
        assert index.dtype == torch.int32 and index.is_cuda and index.is_contiguous() and index.dim() == 1
        if not isinstance(steps, int):
            return self._gather_steps(index, tuple(sorted({int(s) for s in steps})))
        M, K, S, H = index.numel(), int(steps), env.b.n_players, env.b.height
        assert 1 <= K <= self.k_step + 1, "steps outside [1, k_step + 1]"
        if (M, K) not in self._batches:
            u8, f32 = dict(dtype=torch.uint8, device=env.dev), dict(dtype=torch.float32, device=env.dev)
            kind = namedtuple("TrajectoryBatch", "visual vector piece action prob adv target reward done valid")
            t = kind(torch.zeros(S, M, K, H, 10, **u8), torch.zeros(S, M, K, 12, **u8), torch.zeros(S, M, K, **u8), torch.zeros(M, K, 3, **u8),
                     torch.zeros(M, K, **f32), torch.zeros(M, K, **f32), torch.zeros(M, K, **f32), torch.zeros(M, K, **f32), torch.zeros(M, K, **u8),
                     torch.zeros(M, K, **u8))
            self._batches[(M, K)] = (t, env.b.traj_batch(*[env._ptr(x) for x in t]))
        t, out = self._batches[(M, K)]
        env.b.replay_gather_dev(self._rp, env._ptr(index), M, K, out)
        return t

    def _gather_steps(self, index, steps):
        from collections import namedtuple
        from . import capi
        env, torch = self.env, self.env.torch
        M, K, S, H = index.numel(), len(steps), env.b.n_players, env.b.height
        assert K >= 1 and 0 <= steps[0] and steps[-1] <= self.k_step <= 63, "steps outside [0, k_step], or k_step above 63"
        if (M, steps) not in self._batches:
            u8, f32 = dict(dtype=torch.uint8, device=env.dev), dict(dtype=torch.float32, device=env.dev)
            kind = namedtuple("TrajectoryBatch", "visual vector piece action prob adv target reward done valid")
            t = kind(torch.zeros(S, M, K, H, 10, **u8), torch.zeros(S, M, K, 12, **u8), torch.zeros(S, M, K, **u8), torch.zeros(M, K, 3, **u8),
                     torch.zeros(M, K, **f32), torch.zeros(M, K, **f32), torch.zeros(M, K, **f32), torch.zeros(M, K, **f32), torch.zeros(M, K, **u8),
                     torch.zeros(M, K, **u8))
            self._batches[(M, steps)] = (t, env.b.traj_batch(*[env._ptr(x) for x in t]), capi.kstep_mask(steps))
        t, out, mask = self._batches[(M, steps)]
        env.b.replay_gather_steps_dev(self._rp, env._ptr(index), M, mask, out)
        return t

    def inputs(self, index, steps=1, items=("cumsum", "shadow", "height", "holes"), pad=True, dtype=None, channels_last=False):
        """The network's first-layer inputs of the k-step views of index, straight from the ring's records (tetris_net_input_dev):
        index and steps — a count, or a sequence of step numbers — as for gather.  -> (visual [S, M, steps, C, Hp, Wp], vector [S, M,
        steps, 12], piece uint8 [S, M, steps], valid uint8 [M, steps]) as Trajectory.inputs gives them; reused device tensors."""
        from . import capi
        env, torch = self.env, self.env.torch
        assert index.dtype == torch.int32 and index.is_cuda and index.is_contiguous() and index.dim() == 1
        M = index.numel()
        if isinstance(steps, int):
            K = int(steps)
            assert 1 <= K <= self.k_step + 1, "steps outside [1, k_step + 1]"
            source = dict(steps=K)
        else:
            steps = tuple(sorted({int(s) for s in steps}))
            K = len(steps)
            assert K >= 1 and 0 <= steps[0] and steps[-1] <= self.k_step <= 63, "steps outside [0, k_step], or k_step above 63"
            source = dict(step_mask=capi.kstep_mask(steps))
        if not hasattr(self, "_inputs"):
            self._inputs = {}
        return env._net_input(self._inputs, steps, (M, K), dict(m=M, replay=self._rp, index=env._ptr(index), **source), items, pad,
                              torch.float32 if dtype is None else dtype, channels_last)

    def targets(self, index, out, steps=None, gamma=0.99, lam=0.9, truncate=False, used_pieces=None, values=False):
        """model.compute_targets for the samples `index` (int32 device tensor [M]) from the reference net's output for their step
        rows: out = Q [M * n, 4, 10, K] (values=True: v [M * n, V]) float32 or float16 for the n steps of `steps` (None: 1..k_step;
        capi.kstep_steps(k, filter)) as gather(index, steps=steps) lays them out.  Rewards and dones are read in the ring behind
        index[j]: they are not gathered.  -> float32 [M], reused per M; an index outside [0, max_size) gives 0.  No host
        synchronisation."""
        if not hasattr(self, "_targets"):
            self._targets = {}
        return self.env._kstep(self._targets, out, self.reward, self.done, index, self.max_size, self.k_step, steps, gamma, lam, truncate,
                               used_pieces, values)

    def update_prios(self, index, prio):
        """prio[index[j]] = prio[j] (update_prios); -1 entries are skipped"""
        torch = self.env.torch
        assert index.dtype == torch.int32 and index.is_cuda and index.is_contiguous() and index.dim() == 1
        assert prio.dtype == torch.float32 and prio.is_cuda and prio.is_contiguous() and prio.numel() == index.numel()
        self.env.b.replay_update_prios_dev(self._rp, self.env._ptr(index), self.env._ptr(prio), index.numel())

    def __len__(self):
        return int(self.cursor[1].item())

    def dropped(self):
        return int(self.cursor[3].item())
