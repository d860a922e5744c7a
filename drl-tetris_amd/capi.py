"""ctypes binding of libtetris_hip.so (include/tetris_hip.h) — the thin shim between the Python
host code and the HIP kernels.

The library is loaded from ``drl-tetris_amd/lib/libtetris_hip.so`` (built in-tree by
``__graft_entry__.build()``).  There is no CPU path: if the library is missing, or no HIP device is
present, creating a batch raises ``TetrisError``.  (``lib_path`` exists so that the test suite can
point the same binding at its CPU test harness; product code never passes it.)
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(HERE, "lib", "libtetris_hip.so")

MAX_H, W, FIFO_CAP = 32, 10, 16

# the columns of tetris_rt_features_dev / the entries of a policy weight vector (include/tetris_hip.h: TETRIS_POLICY_FEATURES)
POLICY_FEATURE_NAMES = ("lines", "holes", "bumpiness", "aggregate_height", "max_height", "row_transitions", "column_transitions", "wells")

# mirrors `struct tetris_record` (include/tetris_hip.h)
RECORD = np.dtype(
    [
        ("field", np.uint8, (MAX_H, W)), ("grid", np.uint8, (4, 4)), ("x", np.int8), ("y", np.int8),
        ("piece", np.uint8), ("tile", np.uint8), ("spawn_rot", np.uint8), ("cur_rot", np.uint8), ("big", np.uint8),
        ("next", np.uint8), ("dead", np.uint8), ("reward", np.uint8), ("inc_count", np.uint8), ("combo_count", np.uint8),
        ("combo_remaining", np.uint16), ("lock_armed", np.uint8), ("fifo_len", np.uint8), ("line_count", np.uint8),
        ("fifo_overflow", np.uint8), ("time_ms", np.int32), ("incoming", np.float32), ("drop_delay", np.int32),
        ("drop_time", np.int32), ("speedup_time", np.int32), ("lock_time", np.int32), ("min_remaining", np.int32),
        ("combo_start", np.int32), ("combo_time", np.int32), ("fifo_delay", np.int32, (FIFO_CAP,)),
        ("fifo_count", np.int16, (FIFO_CAP,)), ("lines_sent", np.uint16), ("lines_cleared", np.uint16),
        ("lines_blocked", np.uint16), ("garbage_cleared", np.uint16), ("max_combo", np.uint16),
        ("lines_cleared_seen", np.uint16), ("weights", np.float32, (7,)), ("piece_draws", np.uint32),
        ("hole_draws", np.uint32),
    ],
    align=True,
)


# the modes of tetris_select_eval_dev (include/tetris_hip.h: TETRIS_ACT_*)
ACT_MODES = {"argmax": 0, "pi": 1, "rank": 2, "epsilon": 3}


class ActEval(C.Structure):
    """mirrors `struct tetris_act_eval` (include/tetris_hip.h)"""
    _fields_ = [("d_action_eval", C.c_void_p), ("d_state_eval", C.c_void_p), ("n_pieces", C.c_int), ("n_values", C.c_int),
                ("mode", C.c_int), ("flags", C.c_int), ("sample_seed", C.c_uint32), ("reserved", C.c_uint32), ("draw", C.c_uint64),
                ("epsilon", C.c_float), ("table", C.c_void_p), ("d_player", C.c_void_p), ("d_rot", C.c_void_p), ("d_trans", C.c_void_p),
                ("d_piece", C.c_void_p), ("d_eval", C.c_void_p), ("d_value", C.c_void_p), ("d_entropy", C.c_void_p)]


PLAN_OUT_F16 = 4              # TETRIS_PLAN_OUT_F16


class PlanEval(C.Structure):
    """mirrors `struct tetris_plan_eval` (include/tetris_hip.h)"""
    _fields_ = [("d_phi", C.c_void_p), ("d_state_eval", C.c_void_p), ("n_pieces", C.c_int), ("n_values", C.c_int), ("mode", C.c_int),
                ("flags", C.c_int), ("sample_seed", C.c_uint32), ("reserved", C.c_uint32), ("draw", C.c_uint64), ("small_fill", C.c_float),
                ("d_player", C.c_void_p), ("d_count", C.c_void_p), ("d_cols", C.c_void_p), ("max_lists", C.c_int), ("d_choice", C.c_void_p),
                ("d_piece", C.c_void_p), ("d_prob", C.c_void_p), ("d_probs", C.c_void_p), ("d_value", C.c_void_p), ("d_entropy", C.c_void_p),
                ("d_delta", C.c_void_p), ("d_sums", C.c_void_p)]


class Traj(C.Structure):
    """mirrors `struct tetris_traj` (include/tetris_hip.h)"""
    _fields_ = [("capacity", C.c_int), ("reserved", C.c_int), ("d_action", C.c_void_p), ("d_prob", C.c_void_p), ("d_value", C.c_void_p),
                ("d_reward", C.c_void_p), ("d_done", C.c_void_p)]


class TrajObs(C.Structure):
    """mirrors `struct tetris_traj_obs` (include/tetris_hip.h)"""
    _fields_ = [("capacity", C.c_int), ("reserved", C.c_int), ("d_obs", C.c_void_p)]


class TrajBatch(C.Structure):
    """mirrors `struct tetris_traj_batch` (include/tetris_hip.h)"""
    _fields_ = [("d_visual", C.c_void_p), ("d_vector", C.c_void_p), ("d_piece", C.c_void_p), ("d_action", C.c_void_p), ("d_prob", C.c_void_p),
                ("d_adv", C.c_void_p), ("d_target", C.c_void_p), ("d_reward", C.c_void_p), ("d_done", C.c_void_p), ("d_valid", C.c_void_p)]


class TrajPlan(C.Structure):
    """mirrors `struct tetris_traj_plan` (include/tetris_hip.h)"""
    _fields_ = [("capacity", C.c_int), ("reserved", C.c_int), ("d_rec", C.c_void_p)]


PLAN_REC_WORDS = 112          # TETRIS_PLAN_REC_WORDS
PLAN_BATCH_F16 = 1            # TETRIS_PLAN_BATCH_F16
SELECT_AUGMENT = 1            # TETRIS_SELECT_AUGMENT
class Replay(C.Structure):
    """mirrors `struct tetris_replay` (include/tetris_hip.h)"""
    _fields_ = [("capacity", C.c_int), ("k_step", C.c_int), ("d_obs", C.c_void_p), ("d_action", C.c_void_p), ("d_prob", C.c_void_p),
                ("d_adv", C.c_void_p), ("d_target", C.c_void_p), ("d_reward", C.c_void_p), ("d_done", C.c_void_p), ("d_flags", C.c_void_p),
                ("d_prio", C.c_void_p), ("d_cursor", C.c_void_p)]


MIRROR_BIT = 1 << 31          # bit 31 of an index of tetris_traj_batch_dev: the mirrored sample

LOSS_STATS = 16               # TETRIS_LOSS_STATS
LOSS_F16, LOSS_VALUE_F16, LOSS_GRAD_F16 = 1, 2, 4          # TETRIS_LOSS_*
# the slots of d_stats (include/tetris_hip.h: loss heads)
PPO_STATS = ("n", "loss", "value_loss", "policy_loss", "entropy_loss", "entropy", "entropy_sq", "entropy_bonus", "values", "values_sq",
             "target_values", "target_values_sq", "clip_saturation", "ratio")
DQN_STATS = ("n", "n_weighted", "loss", "q_val", "q_val_sq", "q_target", "q_target_sq", "new_prio")
PPO_TERMS = ("probability", "ratio", "policy_term", "entropy", "entropy_bonus", "value")
PLAN_LOSS_STATS = ("n", "loss", "value_loss", "policy_loss", "entropy_loss", "impossibility_loss", "entropy", "entropy_sq", "values",
                   "values_sq", "target_values", "target_values_sq", "clip_saturation", "ratio", "probability")
PLAN_LOSS_TERMS = ("probability", "ratio", "policy_term", "entropy", "impossibility", "value")


class PpoLoss(C.Structure):
    """mirrors `struct tetris_ppo_loss` (include/tetris_hip.h)"""
    _fields_ = [("d_pi", C.c_void_p), ("d_v", C.c_void_p), ("d_action", C.c_void_p), ("d_prob_old", C.c_void_p), ("d_adv", C.c_void_p),
                ("d_target", C.c_void_p), ("d_valid", C.c_void_p), ("M", C.c_int), ("n_pieces", C.c_int), ("n_values", C.c_int),
                ("flags", C.c_int), ("clip", C.c_float), ("value_loss", C.c_float), ("policy_loss", C.c_float), ("entropy_loss", C.c_float),
                ("entropy_floor_loss", C.c_float), ("rescaled_entropy", C.c_float), ("entropy_floor", C.c_float), ("max_entropy", C.c_float),
                ("grad_scale", C.c_float), ("reserved", C.c_float), ("d_grad_pi", C.c_void_p), ("d_grad_v", C.c_void_p),
                ("d_terms", C.c_void_p), ("d_stats", C.c_void_p)]


class PlanLoss(C.Structure):
    """mirrors `struct tetris_plan_loss` (include/tetris_hip.h)"""
    _fields_ = [("d_phi", C.c_void_p), ("d_v", C.c_void_p), ("d_index", C.c_void_p), ("d_piece", C.c_void_p), ("d_prob_old", C.c_void_p),
                ("d_adv", C.c_void_p), ("d_target", C.c_void_p), ("d_valid", C.c_void_p), ("M", C.c_int), ("n_pieces", C.c_int),
                ("n_values", C.c_int), ("flags", C.c_int), ("piece_stride", C.c_int), ("small_fill", C.c_float), ("clip", C.c_float),
                ("value_loss", C.c_float), ("policy_loss", C.c_float), ("entropy_loss", C.c_float), ("impossibility_loss", C.c_float),
                ("grad_scale", C.c_float), ("d_grad_phi", C.c_void_p), ("d_grad_v", C.c_void_p), ("d_terms", C.c_void_p),
                ("d_stats", C.c_void_p)]


class DqnLoss(C.Structure):
    """mirrors `struct tetris_dqn_loss` (include/tetris_hip.h)"""
    _fields_ = [("d_Q", C.c_void_p), ("d_action", C.c_void_p), ("d_target", C.c_void_p), ("d_weight", C.c_void_p), ("d_valid", C.c_void_p),
                ("M", C.c_int), ("n_pieces", C.c_int), ("flags", C.c_int), ("optimistic_prios", C.c_float), ("grad_scale", C.c_float),
                ("reserved", C.c_float), ("d_grad_Q", C.c_void_p), ("d_new_prio", C.c_void_p), ("d_q", C.c_void_p), ("d_stats", C.c_void_p)]


KSTEP_Q, KSTEP_V, KSTEP_TRUNCATE = 0, 1, 8          # TETRIS_KSTEP_*


class KstepTarget(C.Structure):
    """mirrors `struct tetris_kstep_target` (include/tetris_hip.h)"""
    _fields_ = [("d_out", C.c_void_p), ("d_reward", C.c_void_p), ("d_done", C.c_void_p), ("d_index", C.c_void_p), ("M", C.c_int),
                ("k_step", C.c_int), ("step_mask", C.c_uint64), ("max_size", C.c_int), ("mode", C.c_int), ("n_pieces", C.c_int),
                ("n_values", C.c_int), ("used_pieces", C.c_int), ("flags", C.c_int), ("gamma", C.c_float), ("lam", C.c_float),
                ("d_target", C.c_void_p), ("d_values", C.c_void_p), ("d_done_time", C.c_void_p)]


HEAD_MEAN, HEAD_MAX, HEAD_NONE = 0, 1, 2              # TETRIS_HEAD_MEAN / _MAX / _NONE
HEAD_F16, HEAD_VALUE_F16 = 1, 2                        # TETRIS_HEAD_F16 / _VALUE_F16
HEAD_MODES = {"mean": HEAD_MEAN, "max": HEAD_MAX}      # any other string: normalize_advantages' fall-through, HEAD_NONE


class QHead(C.Structure):
    """mirrors `struct tetris_q_head` (include/tetris_hip.h)"""
    _fields_ = [("d_a", C.c_void_p), ("d_v", C.c_void_p), ("d_grad_Q", C.c_void_p), ("M", C.c_int), ("n_pieces", C.c_int),
                ("n_values", C.c_int), ("mode", C.c_int), ("separate_piece_values", C.c_int), ("used_pieces", C.c_int), ("flags", C.c_int),
                ("advantage_range", C.c_float), ("d_Q", C.c_void_p), ("d_V", C.c_void_p), ("d_A", C.c_void_p), ("d_grad_a", C.c_void_p),
                ("d_grad_v", C.c_void_p)]


class PolicyHead(C.Structure):
    """mirrors `struct tetris_policy_head` (include/tetris_hip.h)"""
    _fields_ = [("d_x", C.c_void_p), ("d_w", C.c_void_p), ("d_grad_pi", C.c_void_p), ("d_grad_v", C.c_void_p), ("M", C.c_int),
                ("n_pieces", C.c_int), ("n_values", C.c_int), ("flags", C.c_int), ("d_pi", C.c_void_p), ("d_v", C.c_void_p),
                ("d_grad_x", C.c_void_p), ("d_grad_w", C.c_void_p)]


INPUT_ITEMS = {"cumsum": 1, "shadow": 2, "height": 3, "holes": 4}          # TETRIS_INPUT_CUMSUM / _SHADOW / _HEIGHT / _HOLES
INPUT_F16, INPUT_CHANNELS_LAST, INPUT_PAD = 1, 2, 4                        # TETRIS_INPUT_*


class NetInput(C.Structure):
    """mirrors `struct tetris_net_input` (include/tetris_hip.h)"""
    _fields_ = [("obs", C.c_void_p), ("replay", C.c_void_p), ("d_index", C.c_void_p), ("row", C.c_int), ("M", C.c_int), ("steps", C.c_int),
                ("n_items", C.c_int), ("step_mask", C.c_uint64), ("items", C.c_int * 4), ("flags", C.c_int), ("reserved", C.c_int),
                ("d_visual", C.c_void_p), ("d_vector", C.c_void_p), ("d_piece", C.c_void_p), ("d_valid", C.c_void_p)]


KBD_F16 = 1                                            # TETRIS_KBD_F16
KBD_BLOCK, KBD_W_SAMPLES = 16, 256                     # drl-tetris_amd/csrc/tetris_kbd.h: samples per workgroup, per partial of grad_w


class KbdConv(C.Structure):
    """mirrors `struct tetris_kbd_conv` (include/tetris_hip.h)"""
    _fields_ = [("d_x", C.c_void_p), ("d_w", C.c_void_p), ("d_bias", C.c_void_p), ("d_grad_out", C.c_void_p), ("M", C.c_int),
                ("n_pieces", C.c_int), ("height", C.c_int), ("channels", C.c_int), ("flags", C.c_int), ("reserved", C.c_int),
                ("d_out", C.c_void_p), ("d_grad_x", C.c_void_p), ("d_grad_w", C.c_void_p), ("d_grad_b", C.c_void_p)]


RES_F16 = 1                                            # TETRIS_RES_F16
RES_JOIN_NONE, RES_JOIN_ADD, RES_JOIN_TRUNCATE_ADD = 0, 1, 2               # TETRIS_RES_JOIN_*
RES_ACT_NONE, RES_ACT_ELU = 0, 1                       # TETRIS_RES_ACT_*
RES_JOINS = {None: RES_JOIN_NONE, "none": RES_JOIN_NONE, "add": RES_JOIN_ADD, "truncate_add": RES_JOIN_TRUNCATE_ADD}
RES_ACTS = {None: RES_ACT_NONE, "none": RES_ACT_NONE, "elu": RES_ACT_ELU}
RES_ROWS, RES_W_SAMPLES = 8, 64                        # drl-tetris_amd/csrc/tetris_res.h: image rows per workgroup, samples per partial of grad_w


class ResLayer(C.Structure):
    """mirrors `struct tetris_res_layer` (include/tetris_hip.h)"""
    _fields_ = [("d_x", C.c_void_p), ("d_w", C.c_void_p), ("d_bias", C.c_void_p), ("d_y", C.c_void_p), ("d_grad_out", C.c_void_p),
                ("M", C.c_int), ("height", C.c_int), ("in_channels", C.c_int), ("out_channels", C.c_int), ("join", C.c_int),
                ("activation", C.c_int), ("flags", C.c_int), ("reserved", C.c_int),
                ("d_out", C.c_void_p), ("d_grad_x", C.c_void_p), ("d_grad_w", C.c_void_p), ("d_grad_b", C.c_void_p)]


def res_out_channels(in_channels, out_channels, join):
    """Cout of a residual layer: Co without a join, max(Ci, Co) with "add", min(Ci, Co) with "truncate_add" (peephole_join,
    agents/networks/network_utils.py:52-64)."""
    j = RES_JOINS.get(join, join)
    return int(out_channels) if j == RES_JOIN_NONE else max(int(in_channels), int(out_channels)) if j == RES_JOIN_ADD else min(int(in_channels), int(out_channels))


def input_shape(height, n_items, pad=True):
    """(C, Hp, Wp) of the visual output of net_input_dev: 1 + n_items channels, H + 2 rows and 12 columns with pad, else H and 10."""
    return 1 + int(n_items), int(height) + (2 if pad else 0), W + (2 if pad else 0)


def kstep_steps(k, filter=None):
    """The steps the k-step estimator evaluates its net on (value_estimator._create_steps, agents/networks/value_estimator.py:
    90-99): s in 1..k that no f of `filter` divides; None or an empty filter keeps all.  -> a list of ints, ascending."""
    fs = [int(f) for f in (filter if filter is not None else [])]
    return [s for s in range(1, int(k) + 1) if all(s % f != 0 for f in fs)]


def kstep_mask(steps):
    """The step_mask of replay_gather_steps_dev and kstep_target: bit s for every step s (0..63) of `steps`."""
    mask = 0
    for s in steps:
        if not 0 <= int(s) <= 63:
            raise ValueError(f"step {s} outside [0, 63]")
        mask |= 1 << int(s)
    return mask


def ppo_entropy_constants(ppo_epsilon):
    """The two constants of the PPO head's entropy terms, in float64 (agents/networks/ppo_nets.py:175-180): -> (entropy_floor,
    max_entropy) with entropy_floor = -eps log(eps / 39) - (1 - eps) log(1 - eps) and max_entropy = tools.utils.entropy of the
    uniform distribution over the 40 actions, -sum (1/40) log(1/40 + 1e-8).  For eps <= 0 or eps >= 1, where the reference's
    expression is NaN, the floor is 0: the floor term is switched off."""
    eps = float(ppo_epsilon)
    floor = -eps * np.log(eps / 39.0) - (1.0 - eps) * np.log(1.0 - eps) if 0.0 < eps < 1.0 else 0.0
    uniform = np.full(40, 1.0 / 40.0)
    return float(floor), float(-np.sum(uniform * np.log(uniform + 1e-8)))


def pareto_table(theta):
    """The RANK table of the reference's pareto (tools/utils.py:88-91): (k + 1) ** -theta for rank k + 1, float32 [40]."""
    return (np.arange(1, 41, dtype=np.float64) ** -float(theta)).astype(np.float32)


def act_entropy(mode, epsilon=0.0, table=None):
    """The entropy the reference reports for the modes whose entropy does not depend on the evaluation (sventon_utils.py:21-45,
    tools/utils.py:93-94): argmax 0; epsilon: of e / 40 everywhere plus 1 - e on one entry, e = min(1, epsilon); rank: of the
    normalised table.  (PI's depends on the map: tetris_select_eval_dev writes it per game.)"""
    entropy = lambda p: float(-np.sum(p * np.log(p + 1e-8)))                  # noqa: E731
    if mode == "argmax":
        return 0.0
    if mode == "epsilon":
        e = min(1.0, float(epsilon))
        p = e * np.full(40, 1.0 / 40)
        p[0] += 1.0 - e
        return entropy(p)
    if mode == "rank":
        t = np.asarray(table, np.float64)
        return entropy(t / t.sum())
    raise ValueError(f"the entropy of mode {mode!r} is a per-game output")


class TetrisError(RuntimeError):
    pass


_libs = {}

_SIGNATURES = {
    "tetris_last_error": (C.c_char_p, []),
    "tetris_device_count": (C.c_int, []),
    "tetris_device_name": (C.c_int, [C.c_int, C.c_char_p, C.c_int]),
    "tetris_record_size": (C.c_int, []),
    "tetris_layout_words": (C.c_int, []),
    "tetris_snapshot_words": (C.c_int, [C.c_void_p]),
    "tetris_table_chunks": (C.c_int, [C.c_void_p]),
    "tetris_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "tetris_create_ex": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    "tetris_destroy": (C.c_int, [C.c_void_p]),
    "tetris_sync": (C.c_int, [C.c_void_p]),
    "tetris_take_errors": (C.c_int, [C.c_void_p, C.c_void_p]),
    "tetris_set_game_offset": (C.c_int, [C.c_void_p, C.c_uint64]),
    "tetris_set_chained": (C.c_int, [C.c_void_p, C.c_int]),
    "tetris_rollout_is_chained": (C.c_int, [C.c_void_p, C.c_int]),
    "tetris_set_direct_dispatch": (C.c_int, [C.c_void_p, C.c_int]),
    "tetris_rollout_was_direct": (C.c_int, [C.c_void_p]),
    "tetris_set_xcd_affine": (C.c_int, [C.c_void_p, C.c_int]),
    "tetris_debug_xcd_skew": (C.c_int, [C.c_void_p, C.c_int]),
    "tetris_debug_table_limit": (C.c_int, [C.c_void_p, C.c_int]),
    "tetris_debug_code_objects": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_uint64)]),
    "tetris_set_chain_spin_limit": (C.c_int, [C.c_void_p, C.c_uint32]),
    "tetris_debug_stall": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "tetris_debug_chain_epoch": (C.c_int, [C.c_void_p, C.c_longlong, C.c_void_p]),
    "tetris_debug_clock_khz": (C.c_int, [C.c_void_p, C.c_void_p]),
    "tetris_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "tetris_make_actions": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]),
    "tetris_finish_actions": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tetris_step_keys": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tetris_step_rt": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tetris_step_rt_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tetris_step_rt_dev_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "tetris_step_rt_observe_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tetris_reset_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "tetris_observe_records": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tetris_snapshot": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "tetris_restore": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "tetris_set_dead": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "tetris_enumerate_drops": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tetris_enumerate_drops_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tetris_enumerate_drops_dev_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "tetris_timer_start": (C.c_int, [C.c_void_p]),
    "tetris_timer_stop": (C.c_int, [C.c_void_p, C.c_void_p]),
    "tetris_get_actions": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "tetris_action_lists_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tetris_simulate_lists_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tetris_step_lists_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.c_void_p, C.c_void_p, C.c_void_p]),
    "tetris_plan_deltas_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_void_p,
                                         C.c_void_p]),
    "tetris_select_lists_dev": (C.c_int, [C.c_void_p, C.c_void_p]),
    "tetris_step_lists_eval_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                             C.c_void_p]),
    "tetris_rt_features_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "tetris_policy_rt_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tetris_step_policy_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p]),
    "tetris_rollout_policy": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p]),
    "tetris_rollout_game_totals_dev": (C.c_int, [C.c_void_p, C.c_void_p]),
    "tetris_select_eval_dev": (C.c_int, [C.c_void_p, C.c_void_p]),
    "tetris_step_eval_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tetris_step_eval_observe_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p]),
    "tetris_traj_record_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tetris_traj_advantages_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p]),
    "tetris_traj_observe_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "tetris_traj_select_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p]),
    "tetris_traj_batch_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "tetris_traj_record_plan_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tetris_traj_plan_batch_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_void_p]),
    "tetris_replay_add_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                        C.c_int]),
    "tetris_replay_sample_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p]),
    "tetris_replay_update_prios_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "tetris_replay_gather_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "tetris_replay_gather_steps_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_void_p]),
    "tetris_kstep_target_dev": (C.c_int, [C.c_void_p, C.c_void_p]),
    "tetris_q_head_dev": (C.c_int, [C.c_void_p, C.c_void_p]),
    "tetris_q_head_grad_dev": (C.c_int, [C.c_void_p, C.c_void_p]),
    "tetris_policy_head_dev": (C.c_int, [C.c_void_p, C.c_void_p]),
    "tetris_policy_head_grad_dev": (C.c_int, [C.c_void_p, C.c_void_p]),
    "tetris_net_input_dev": (C.c_int, [C.c_void_p, C.c_void_p]),
    "tetris_kbd_conv_dev": (C.c_int, [C.c_void_p, C.c_void_p]),
    "tetris_kbd_conv_grad_x_dev": (C.c_int, [C.c_void_p, C.c_void_p]),
    "tetris_kbd_conv_grad_w_dev": (C.c_int, [C.c_void_p, C.c_void_p]),
    "tetris_res_layer_dev": (C.c_int, [C.c_void_p, C.c_void_p]),
    "tetris_res_layer_grad_x_dev": (C.c_int, [C.c_void_p, C.c_void_p]),
    "tetris_res_layer_grad_w_dev": (C.c_int, [C.c_void_p, C.c_void_p]),
    "tetris_ppo_loss_dev": (C.c_int, [C.c_void_p, C.c_void_p]),
    "tetris_dqn_loss_dev": (C.c_int, [C.c_void_p, C.c_void_p]),
    "tetris_plan_loss_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "tetris_observe_packed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tetris_observe_packed_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tetris_create_split": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "tetris_split_stage_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tetris_split_rollout_stage_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p]),
    "tetris_rollout_totals": (C.c_int, [C.c_void_p, C.c_void_p]),
    "tetris_set_stream": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "tetris_rollout_random": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p]),
    "tetris_rollout_launch": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_uint64, C.c_int, C.c_void_p]),
    "tetris_device_state": (C.c_void_p, [C.c_void_p]),
    "tetris_stream": (C.c_void_p, [C.c_void_p]),
}

EXPORTS = tuple(_SIGNATURES)


def _share_hip_runtime_with_torch():
    """One process must use ONE HIP runtime.  PyTorch-ROCm wheels bundle their own libamdhip64; if this library pulled
    in the system copy first, a later `import torch` would load a second runtime and find no GPU.  So when torch is
    installed (not necessarily imported), load its bundled runtime first with RTLD_GLOBAL; libtetris_hip.so's
    libamdhip64 dependency then resolves to it.  Without torch the system ROCm runtime is used."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return                              # torch already loaded its runtime
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    for root in (spec.submodule_search_locations if spec and spec.submodule_search_locations else []):
        cand = os.path.join(root, "lib", "libamdhip64.so")
        if os.path.exists(cand):
            try:
                C.CDLL(cand, mode=C.RTLD_GLOBAL)
            except OSError:
                pass
            return


def load_library(lib_path=None):
    path = os.path.abspath(lib_path or DEFAULT_LIB)
    if path in _libs:
        return _libs[path]
    if lib_path is None:
        _share_hip_runtime_with_torch()
    if not os.path.exists(path):
        raise TetrisError(f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    lib = C.CDLL(path)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError here = the library does not export the ABI
        fn.restype, fn.argtypes = res, args
    if lib.tetris_record_size() != RECORD.itemsize:
        raise TetrisError("tetris_record layout mismatch between the library and capi.RECORD")
    _libs[path] = lib
    return lib


def device_name(device=0, lib_path=None):
    buf = C.create_string_buffer(256)
    rc = load_library(lib_path).tetris_device_name(int(device), buf, 256)
    return buf.value.decode() if rc == 0 else "unknown"


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _u8(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    if shape is not None and a.shape != shape:
        raise ValueError(f"expected shape {shape}, got {a.shape}")
    return a


class TetrisBatch:
    """N games resident on one GPU (one `tetris_batch`)."""

    def __init__(self, n_games, n_players=2, height=20, width=10, pieces=(0, 1, 2, 3, 4, 5, 6), seeds=None, device=0, lib_path=None,
                 split_side=None, colours=False):
        """split_side = 0 / 1: this batch holds only that player of n_games two-player games (opponents on another GPU).
        colours: also track tile values, so that records hold the reference's exact State.field (1..7 tiles, 8 garbage)."""
        self.lib = load_library(lib_path)
        self.split_side = split_side
        if split_side is not None:
            n_players = 1
        self.n_games, self.n_players, self.height, self.width = int(n_games), int(n_players), int(height), int(width)
        self.piece_map = np.array((list(pieces) * 7)[:7], dtype=np.uint8)      # tetris_environment.py:191-193
        self._h = C.c_void_p()
        s = self._seeds(seeds, self.n_games) if seeds is not None else None
        self.colours = bool(colours)
        if split_side is None:
            self._check(self.lib.tetris_create_ex(C.byref(self._h), self.n_games, self.n_players, self.height, self.width,
                                                  _p(self.piece_map), int(device), _p(s), 1 if colours else 0))
        else:
            self._check(self.lib.tetris_create_split(C.byref(self._h), self.n_games, int(split_side), self.height, self.width,
                                                     _p(self.piece_map), int(device), _p(s)))
        self.snapshot_words = self.lib.tetris_snapshot_words(self._h)

    # -- plumbing
    def _check(self, rc):
        if rc != 0:
            raise TetrisError(f"libtetris_hip error {rc}: {self.lib.tetris_last_error().decode()}")

    @staticmethod
    def _seeds(seeds, n):
        # randomizer.cpp:34-36: seeds are truncated to `short`
        return np.ascontiguousarray(np.broadcast_to(np.asarray(seeds), (n,)).astype(np.int64).astype(np.int16))

    def _idx(self, idx):
        if idx is None:
            return None, self.n_games
        a = np.ascontiguousarray(idx, dtype=np.int32).reshape(-1)
        return a, len(a)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.tetris_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- the reference's PythonHandle surface, batched
    def reset(self, idx=None, seeds=0):
        a, n = self._idx(idx)
        self._check(self.lib.tetris_reset(self._h, _p(a), n, _p(self._seeds(seeds, n))))

    def make_actions(self, keys, lens, idx=None):
        a, n = self._idx(idx)
        keys = _u8(keys)
        lens = _u8(lens, (n, self.n_players))
        if keys.ndim != 3 or keys.shape[:2] != (n, self.n_players):
            raise ValueError("keys must be [n, P, max_keys]")
        self._check(self.lib.tetris_make_actions(self._h, _p(a), n, _p(keys), _p(lens), keys.shape[2]))

    def finish_actions(self, ms=400, idx=None, full=False):
        a, n = self._idx(idx)
        done = np.zeros(n, np.uint8)
        lines = np.zeros((n, self.n_players), np.uint8)
        dead = np.zeros((n, self.n_players), np.uint8)
        self._check(self.lib.tetris_finish_actions(self._h, _p(a), n, int(ms), _p(done), _p(lines), _p(dead)))
        return (done, lines, dead) if full else done

    def step_keys(self, keys, lens, ms=400, idx=None):
        a, n = self._idx(idx)
        keys = _u8(keys)
        lens = _u8(lens, (n, self.n_players))
        if keys.ndim != 3 or keys.shape[:2] != (n, self.n_players):
            raise ValueError("keys must be [n, P, max_keys]")
        done = np.zeros(n, np.uint8)
        lines = np.zeros((n, self.n_players), np.uint8)
        dead = np.zeros((n, self.n_players), np.uint8)
        self._check(self.lib.tetris_step_keys(self._h, _p(a), n, _p(keys), _p(lens), keys.shape[2], int(ms), _p(done), _p(lines), _p(dead)))
        return done, lines, dead

    def step_rt(self, rot, trans, player=None, ms=400, full=False):
        n = self.n_games
        rot, trans = _u8(rot, (n,)), _u8(trans, (n,))
        pl = None if player is None else _u8(np.broadcast_to(player, (n,)))
        done = np.zeros(n, np.uint8)
        lines = np.zeros((n, self.n_players), np.uint8)
        dead = np.zeros((n, self.n_players), np.uint8)
        self._check(self.lib.tetris_step_rt(self._h, _p(rot), _p(trans), _p(pl), int(ms), _p(done), _p(lines), _p(dead)))
        return (done, lines, dead) if full else done

    def step_rt_dev(self, rot, trans, player, done, lines, dead, ms=400, auto_reset=False):
        """tetris_step_rt_dev_ex: every argument is a raw DEVICE address (int / c_void_p) or None; only enqueues.
        auto_reset: finished games are reset inside the launch with the next seed of the built-in schedule."""
        self._check(self.lib.tetris_step_rt_dev_ex(self._h, rot, trans, player, int(ms), done, lines, dead, 1 if auto_reset else 0))

    def step_rt_observe_dev(self, rot, trans, player, done, lines, dead, next_player, visual, vector, piece, ms=400, auto_reset=False):
        """tetris_step_rt_observe_dev: the step of step_rt_dev and the packed observation of the stepped state (perspective of
        next_player) in one launch; every argument is a raw DEVICE address or None; only enqueues."""
        self._check(self.lib.tetris_step_rt_observe_dev(self._h, rot, trans, player, int(ms), done, lines, dead, 1 if auto_reset else 0,
                                                        next_player, visual, vector, piece))

    def reset_dev(self, mask=None, seeds=None):
        """tetris_reset_dev: device mask [N] (None = all games), device seeds int16 [N] (None = built-in schedule); only enqueues."""
        self._check(self.lib.tetris_reset_dev(self._h, mask, seeds))

    def observe(self, idx=None):
        a, n = self._idx(idx)
        rec = np.zeros((n, self.n_players), dtype=RECORD)
        ro = np.zeros(n, np.uint8)
        lw = np.zeros(n, np.int8)
        self._check(self.lib.tetris_observe_records(self._h, _p(a), n, _p(rec), _p(ro), _p(lw)))
        return rec, ro, lw

    def observe_packed(self, idx=None, player=None):
        """NN-ready observations (state_dict + unpacker defaults): visual u8 [S,n,H,W], vector u8 [S,n,12], piece u8 [S,n];
        slot 0 = `player`'s own board, slot 1 = the opponent's."""
        a, n = self._idx(idx)
        pl = None if player is None else _u8(np.broadcast_to(player, (n,)))
        S = self.n_players
        visual = np.zeros((S, n, self.height, self.width), np.uint8)
        vector = np.zeros((S, n, 12), np.uint8)
        piece = np.zeros((S, n), np.uint8)
        self._check(self.lib.tetris_observe_packed(self._h, _p(a), n, _p(pl), _p(visual), _p(vector), _p(piece)))
        return visual, vector, piece

    def snapshot(self, idx=None):
        a, n = self._idx(idx)
        blob = np.zeros((n, self.snapshot_words), np.uint32)
        self._check(self.lib.tetris_snapshot(self._h, _p(a), n, _p(blob)))
        return blob

    def restore(self, blob, idx=None):
        a, n = self._idx(idx)
        blob = np.ascontiguousarray(blob, dtype=np.uint32)
        if blob.shape != (n, self.snapshot_words):
            raise ValueError(f"blob must be [{n}, {self.snapshot_words}]")
        self._check(self.lib.tetris_restore(self._h, _p(a), n, _p(blob)))

    def set_dead(self, dead, idx=None):
        a, n = self._idx(idx)
        self._check(self.lib.tetris_set_dead(self._h, _p(a), n, _p(_u8(dead, (n, self.n_players)))))

    def enumerate_drops(self, idx=None, player=None, columns=True):
        """-> valid u8 [n,4,10], land_y i8 [n,4,10], cleared u8 [n,4,10], after u32 [n,4,10,10] column bitboards (or None)"""
        a, n = self._idx(idx)
        pl = None if player is None else _u8(np.broadcast_to(player, (n,)))
        valid = np.zeros((n, 4, 10), np.uint8)
        land = np.zeros((n, 4, 10), np.int8)
        cleared = np.zeros((n, 4, 10), np.uint8)
        after = np.zeros((n, 4, 10, 10), np.uint32) if columns else None
        self._check(self.lib.tetris_enumerate_drops(self._h, _p(a), n, _p(pl), _p(valid), _p(land), _p(cleared), _p(after)))
        return valid, land, cleared, after

    def enumerate_drops_dev(self, n, valid, land_y, cleared, after=None, idx=None, player=None, planar=False):
        """tetris_enumerate_drops_dev_ex: raw DEVICE addresses (int / c_void_p) or None; only enqueues.
        planar: rotation-minor planes — valid / land_y / cleared [n][10][4], after [10][n][10][4]."""
        self._check(self.lib.tetris_enumerate_drops_dev_ex(self._h, idx, int(n), player, valid, land_y, cleared, after, 1 if planar else 0))

    def get_actions(self, idx=None, player=None, max_lists=64, max_keys=48, with_masks=False):
        """The reference's ordered key lists per game (PythonHandle.get_actions; masks[p].action).
        `idx` may be an int (one game -> one list of lists) or None/array (-> list per game)."""
        single = isinstance(idx, (int, np.integer))
        a, n = self._idx([idx] if single else idx)
        pl = None if player is None else _u8(np.broadcast_to(player, (n,)))
        keys = np.zeros((n, max_lists, max_keys), np.uint8)
        lens = np.zeros((n, max_lists), np.uint8)
        count = np.zeros(n, np.int32)
        self._check(self.lib.tetris_get_actions(self._h, _p(a), n, _p(pl), _p(keys), _p(lens), _p(count), max_lists, max_keys))
        out = [[keys[i, k, : lens[i, k]].tolist() for k in range(count[i])] for i in range(n)]
        if with_masks:
            # PythonHandle.masks[p].mask after get_actions (PythonHandle.h:317-325): TestField::getMask(2) pushes one 1 per key list
            # (TestField.cpp:113-133), i.e. a vector of ones as long as the list of actions — probed against the compiled reference
            masks = [[1] * int(c) for c in count]
            return (out[0], masks[0]) if single else (out, masks)
        return out[0] if single else out

    # -- planning on the device (include/tetris_hip.h: tetris_action_lists_dev and the three after it).  Every array argument is
    # a raw DEVICE address (int / c_void_p) or None; these only enqueue.  Lists: count int32 [N], lens uint8 [N][L],
    # keys uint8 [N][L][K].
    def action_lists_dev(self, count, lens, keys, max_lists=64, max_keys=48, player=None, keep_null=False):
        """get_actions(player) + action_list(remove_null=not keep_null) for every game (count -1: did not fit, TETRIS_ERR_LISTS)."""
        self._check(self.lib.tetris_action_lists_dev(self._h, player, int(max_lists), int(max_keys), 1 if keep_null else 0, count, lens, keys))

    def simulate_lists_dev(self, count, lens, keys, cols, max_lists=64, max_keys=48, player=None, finalize=False, ms=400,
                           done=None, lines=None, dead=None):
        """simulate_actions of every list: cols uint32 [L][P][10][N]; with finalize also done [L][N], lines / dead [L][P][N]."""
        self._check(self.lib.tetris_simulate_lists_dev(self._h, player, count, lens, keys, int(max_lists), int(max_keys), int(ms),
                                                       1 if finalize else 0, cols, done, lines, dead))

    def step_lists_dev(self, choice, count, lens, keys, done, lines, dead, max_lists=64, max_keys=48, player=None, ms=400, auto_reset=False):
        """perform_action(lists[choice[i]], player) for every game: choice int32 [N]; done [N], lines / dead [P][N]."""
        self._check(self.lib.tetris_step_lists_dev(self._h, player, choice, count, lens, keys, int(max_lists), int(max_keys), int(ms),
                                                   1 if auto_reset else 0, done, lines, dead))

    def plan_deltas_dev(self, count, cols, deltas, sums=None, small=None, max_lists=64, player=None, small_fill=1e-3, f16=False,
                        list_major=False):
        """sherlock_utils.generate_deltas from the columns simulate_lists_dev(finalize=False) wrote: deltas float32 [N][H][10][L]
        (list_major: [N][L][H][10]; f16: binary16), sums N x H x 10 (or None), small uint8 [N][L] (or None); deltas / sums
        16-byte aligned, max_lists <= 256."""
        self._check(self.lib.tetris_plan_deltas_dev(self._h, player, count, cols, int(max_lists), float(small_fill),
                                                    (1 if f16 else 0) | (2 if list_major else 0), deltas, sums, small))

    # -- choosing a planning agent's list from phi (include/tetris_hip.h: tetris_select_lists_dev, tetris_step_lists_eval_dev)
    def plan_eval(self, phi, count, cols, choice, n_pieces=7, f16=False, state_eval=None, n_values=1, value_f16=False, mode="argmax",
                  player=None, seed=0, draw=0, small_fill=1e-3, max_lists=64, out_f16=False, piece=None, prob=None, probs=None, value=None,
                  entropy=None, delta=None, sums=None, flags=0):
        """The argument struct of the two calls below.  Array arguments are raw DEVICE addresses (int / c_void_p) or None.  mode:
        "argmax" or "pi" (or a number).  phi [N][H][10][n_pieces] float32 (f16: binary16), state_eval [N][n_values]; count int32 [N],
        cols uint32 [L][P][10][N] as simulate_lists_dev(finalize=False) wrote them; choice int32 [N], piece uint8 [N], prob float32
        [N], probs float32 [N][L], value float32 [2][N], entropy float32 [N] (PI), delta / sums [N][H][10] float32 (out_f16:
        binary16); phi / delta / sums 16-byte aligned, max_lists <= 256."""
        val = lambda a: a.value if isinstance(a, C.c_void_p) else a               # noqa: E731
        e = PlanEval()
        e.d_phi, e.d_state_eval, e.n_pieces, e.n_values = val(phi), val(state_eval), int(n_pieces), int(n_values)
        e.mode = ACT_MODES[mode] if isinstance(mode, str) else int(mode)
        e.flags = (1 if f16 else 0) | (2 if value_f16 else 0) | (PLAN_OUT_F16 if out_f16 else 0) | int(flags)
        e.sample_seed, e.draw, e.small_fill = int(seed) & 0xFFFFFFFF, int(draw), float(small_fill)
        e.d_player, e.d_count, e.d_cols, e.max_lists = val(player), val(count), val(cols), int(max_lists)
        e.d_choice, e.d_piece, e.d_prob, e.d_probs = val(choice), val(piece), val(prob), val(probs)
        e.d_value, e.d_entropy, e.d_delta, e.d_sums = val(value), val(entropy), val(delta), val(sums)
        return e

    def select_lists_dev(self, e):
        """The list of every game chosen from the network's phi (e = plan_eval(...)); the games are not changed."""
        self._check(self.lib.tetris_select_lists_dev(self._h, C.byref(e) if e is not None else None))

    def step_lists_eval_dev(self, e, lens, keys, done, lines, dead, max_keys=48, ms=400, auto_reset=False):
        """select_lists_dev + step_lists_dev with its choice in one call: done [N], lines / dead [P][N] (each may be None)."""
        self._check(self.lib.tetris_step_lists_eval_dev(self._h, C.byref(e) if e is not None else None, lens, keys, int(max_keys), int(ms),
                                                        1 if auto_reset else 0, done, lines, dead))

    # -- heuristic policy on the device (include/tetris_hip.h: tetris_rt_features_dev and the four after it).  Array arguments
    # are raw DEVICE addresses (int / c_void_p) or None; weights: int16 [8], or [N][8] with per_game.
    def rt_features_dev(self, features, player=None):
        """The POLICY_FEATURE_NAMES features of the 40 (r, t) candidate fields of every game: features int16 [40][8][N]."""
        self._check(self.lib.tetris_rt_features_dev(self._h, player, features))

    def policy_rt_dev(self, weights, rot, trans, score=None, player=None, per_game=False):
        """The best-scoring (r, t) of every game (lowest 10 r + t among equals): rot / trans uint8 [N], score int32 [N] or None."""
        self._check(self.lib.tetris_policy_rt_dev(self._h, player, weights, 1 if per_game else 0, rot, trans, score))

    def step_policy_dev(self, weights, done, lines, dead, rot=None, trans=None, player=None, per_game=False, ms=400, auto_reset=False):
        """policy_rt_dev + step_rt_dev in one call: done [N], lines / dead [P][N]; rot / trans [N] (or None) report what was played."""
        self._check(self.lib.tetris_step_policy_dev(self._h, player, weights, 1 if per_game else 0, int(ms), 1 if auto_reset else 0,
                                                    done, lines, dead, rot, trans))

    def rollout_policy(self, weights, launches, steps_per_launch=1, per_game=False, first_step=0, ms=400):
        """rollout_random with the heuristic policy in place of the random draw; weights: a raw DEVICE address.
        -> (counters[4] = env_steps, episodes, lines, sent; elapsed_ms on the batch's stream)"""
        counters = np.zeros(4, np.uint64)
        elapsed = C.c_float(0.0)
        self._check(self.lib.tetris_rollout_policy(self._h, int(launches), int(steps_per_launch), weights, 1 if per_game else 0,
                                                   int(first_step), int(ms), _p(counters), C.byref(elapsed)))
        return counters, float(elapsed.value)

    # -- acting on a network's (r, t, piece) evaluation (include/tetris_hip.h: tetris_select_eval_dev and the two after it)
    def act_eval(self, action_eval, rot, trans, n_pieces=7, f16=False, state_eval=None, n_values=1, value_f16=False, mode="argmax",
                 player=None, seed=0, draw=0, epsilon=0.0, table=None, piece=None, eval=None, value=None, entropy=None, flags=0):
        """The argument struct of the three calls below.  Array arguments are raw DEVICE addresses (int / c_void_p) or None, but
        `table`: a host float32 [40] array (RANK; pareto_table(theta) gives the reference's).  mode: a key of ACT_MODES or a number.
        action_eval [N][4][10][n_pieces] float32 (f16: binary16), state_eval [N][n_values]; rot / trans / piece uint8 [N], eval
        float32 [N], value float32 [2][N], entropy float32 [N] (PI)."""
        val = lambda a: a.value if isinstance(a, C.c_void_p) else a               # noqa: E731
        e = ActEval()
        e.d_action_eval, e.d_state_eval, e.n_pieces, e.n_values = val(action_eval), val(state_eval), int(n_pieces), int(n_values)
        e.mode = ACT_MODES[mode] if isinstance(mode, str) else int(mode)
        e.flags = (1 if f16 else 0) | (2 if value_f16 else 0) | int(flags)
        e.sample_seed, e.draw, e.epsilon = int(seed) & 0xFFFFFFFF, int(draw), float(epsilon)
        if table is not None:
            e._table = np.ascontiguousarray(table, dtype=np.float32)             # kept alive with the struct
            if e._table.shape != (40,):
                raise ValueError("table must hold 40 float32")
            e.table = e._table.ctypes.data
        e.d_player, e.d_rot, e.d_trans, e.d_piece = val(player), val(rot), val(trans), val(piece)
        e.d_eval, e.d_value, e.d_entropy = val(eval), val(value), val(entropy)
        return e

    def select_eval_dev(self, e):
        """The choice of every game from the network's evaluation (e = act_eval(...)); the games are not changed."""
        self._check(self.lib.tetris_select_eval_dev(self._h, C.byref(e) if e is not None else None))

    def step_eval_dev(self, e, done, lines, dead, ms=400, auto_reset=False):
        """select_eval_dev + step_rt_dev in one call: done [N], lines / dead [P][N] (each may be None)."""
        self._check(self.lib.tetris_step_eval_dev(self._h, C.byref(e) if e is not None else None, int(ms), 1 if auto_reset else 0,
                                                  done, lines, dead))

    def step_eval_observe_dev(self, e, done, lines, dead, next_player, visual, vector, piece, ms=400, auto_reset=False):
        """step_eval_dev and the packed observation of the stepped state (perspective of next_player), as step_rt_observe_dev."""
        self._check(self.lib.tetris_step_eval_observe_dev(self._h, C.byref(e) if e is not None else None, int(ms), 1 if auto_reset else 0,
                                                          done, lines, dead, next_player, visual, vector, piece))

    # -- trajectory windows (include/tetris_hip.h: tetris_traj_record_dev, tetris_traj_advantages_dev)
    def traj(self, capacity, action, prob, value, reward, done):
        """The window struct of the two calls below over raw DEVICE addresses (int / c_void_p): action uint8 [T][N][4], prob
        float32 [T][N], value float32 [2][T][N], reward float32 [T][N], done uint8 [T][N], T = capacity."""
        val = lambda a: a.value if isinstance(a, C.c_void_p) else a               # noqa: E731
        t = Traj()
        t.capacity, t.reserved = int(capacity), 0
        t.d_action, t.d_prob, t.d_value, t.d_reward, t.d_done = val(action), val(prob), val(value), val(reward), val(done)
        return t

    def traj_record_dev(self, traj, row, e, done, dead):
        """Row `row` of the window from the outputs of the acting call e = act_eval(...) and the step's done [N], dead [P][N]."""
        self._check(self.lib.tetris_traj_record_dev(self._h, C.byref(traj) if traj is not None else None, int(row),
                                                    C.byref(e) if e is not None else None, done, dead))

    def traj_advantages_dev(self, traj, rows, gamma, lambda_adv, lambda_value, boot, adv, target, closed=None):
        """Advantages and value targets of rows 0 .. rows-1: adv, target float32 [rows][N], closed uint8 [rows][N] or None, boot
        float32 [N] or None."""
        self._check(self.lib.tetris_traj_advantages_dev(self._h, C.byref(traj) if traj is not None else None, int(rows), float(gamma),
                                                        float(lambda_adv), float(lambda_value), boot, adv, target, closed))

    # -- a window's states and sample sets (include/tetris_hip.h: tetris_traj_observe_dev, tetris_traj_select_dev, tetris_traj_batch_dev)
    def traj_obs(self, capacity, obs):
        """The record struct of the calls below over a raw DEVICE address: obs uint32 [T][N][S][12], 16-byte aligned."""
        o = TrajObs()
        o.capacity, o.reserved, o.d_obs = int(capacity), 0, (obs.value if isinstance(obs, C.c_void_p) else obs)
        return o

    def traj_batch(self, visual=None, vector=None, piece=None, action=None, prob=None, adv=None, target=None, reward=None, done=None,
                   valid=None):
        """The output struct of traj_batch_dev over raw DEVICE addresses (None: that output is skipped): visual uint8 [S][M][H][10],
        vector uint8 [S][M][12], piece uint8 [S][M], action uint8 [M][3], prob / adv / target / reward float32 [M], done / valid
        uint8 [M]."""
        val = lambda a: a.value if isinstance(a, C.c_void_p) else a               # noqa: E731
        o = TrajBatch()
        o.d_visual, o.d_vector, o.d_piece, o.d_action, o.d_prob = val(visual), val(vector), val(piece), val(action), val(prob)
        o.d_adv, o.d_target, o.d_reward, o.d_done, o.d_valid = val(adv), val(target), val(reward), val(done), val(valid)
        return o

    def traj_observe_dev(self, obs, row, player=None):
        """Row `row` of the records from the games' current state, perspective of player [N] (None: player 0)."""
        self._check(self.lib.tetris_traj_observe_dev(self._h, C.byref(obs) if obs is not None else None, int(row), player))

    def traj_select_dev(self, mask, rows, index, cap, count, augment=False):
        """The flat indices of the non-zero bytes of mask uint8 [rows][N], ascending, into index int32 [cap] (-1 past the list;
        augment: the list once more with bit 31 set); count int32 [1] = the length of the full list."""
        self._check(self.lib.tetris_traj_select_dev(self._h, mask, int(rows), SELECT_AUGMENT if augment else 0, index, int(cap), count))

    def traj_batch_dev(self, traj, obs, index, m, out, adv=None, target=None):
        """The samples index int32 [m] names (bit 31: mirrored; -1 or out of range: zeros, valid 0) into out = traj_batch(...);
        adv / target float32 [T][N] or None."""
        self._check(self.lib.tetris_traj_batch_dev(self._h, C.byref(traj) if traj is not None else None,
                                                   C.byref(obs) if obs is not None else None, adv, target, index, int(m),
                                                   C.byref(out) if out is not None else None))

    # -- the planning agent's windows (include/tetris_hip.h: tetris_traj_record_plan_dev, tetris_traj_plan_batch_dev)
    def traj_plan(self, capacity, rec):
        """The record struct of the two calls below over a raw DEVICE address: rec uint32 [T][N][112], 16-byte aligned."""
        o = TrajPlan()
        o.capacity, o.reserved, o.d_rec = int(capacity), 0, (rec.value if isinstance(rec, C.c_void_p) else rec)
        return o

    def traj_record_plan_dev(self, traj, plan, obs, row, e, done, dead):
        """Row `row` of the window and of its plan records from the choosing call e = plan_eval(...) that has just been used, the
        row of obs that traj_observe_dev wrote before it, and the step's done [N], dead [P][N].  plan None: the row arrays only."""
        ref = lambda s: C.byref(s) if s is not None else None                     # noqa: E731
        self._check(self.lib.tetris_traj_record_plan_dev(self._h, ref(traj), ref(plan), ref(obs), int(row), ref(e), done, dead))

    def traj_plan_batch_dev(self, plan, index, m, delta=None, sums=None, small_fill=1e-3, f16=False, flags=0):
        """delta / sums [m][H][10] float32 (f16: binary16; 16-byte aligned, either may be None) of the entries index int32 [m]
        names (bit 31: mirrored; -1 or out of range: zeros)."""
        self._check(self.lib.tetris_traj_plan_batch_dev(self._h, C.byref(plan) if plan is not None else None, index, int(m), float(small_fill),
                                                        (PLAN_BATCH_F16 if f16 else 0) | int(flags), delta, sums))

    # -- experience replay (include/tetris_hip.h: tetris_replay_add_dev and the three after it)
    def replay(self, capacity, k_step, obs, action, prob, adv, target, reward, done, flags, prio, cursor):
        """The buffer struct of the four calls below over raw DEVICE addresses: obs uint32 [C][S][12] (16-byte aligned), action
        uint8 [C][4], prob / adv / target / reward float32 [C], done / flags uint8 [C], prio float32 [C - k_step], cursor int32
        [4]; C = capacity.  The caller zeroes them once."""
        val = lambda a: a.value if isinstance(a, C.c_void_p) else a               # noqa: E731
        r = Replay()
        r.capacity, r.k_step = int(capacity), int(k_step)
        r.d_obs, r.d_action, r.d_prob, r.d_adv, r.d_target = val(obs), val(action), val(prob), val(adv), val(target)
        r.d_reward, r.d_done, r.d_flags, r.d_prio, r.d_cursor = val(reward), val(done), val(flags), val(prio), val(cursor)
        return r

    def replay_add_dev(self, rp, traj, obs, mask, rows, adv=None, target=None, prio=None, augment=False):
        """The entries of mask uint8 [rows][N] of the window (traj, obs; adv / target / prio float32 [T][N] or None) into the
        ring, game-major; augment: every game's run once more, flagged as mirrored.  The cursor moves on the device."""
        ref = lambda x: C.byref(x) if x is not None else None                     # noqa: E731
        self._check(self.lib.tetris_replay_add_dev(self._h, ref(rp), ref(traj), ref(obs), adv, target, prio, mask, int(rows),
                                                   SELECT_AUGMENT if augment else 0))

    def replay_sample_dev(self, rp, m, alpha, beta, seed, draw, index, weight, count, rank=None, key=None):
        """Rank-based prioritised sampling without replacement: index int32 [m] (-1 past min(m, n)), weight float32 [m], count int32
        [1]; rank int32 / key float32 [max_size] or None."""
        self._check(self.lib.tetris_replay_sample_dev(self._h, C.byref(rp) if rp is not None else None, int(m), float(alpha), float(beta),
                                                      int(seed) & 0xFFFFFFFF, int(draw) & 0xFFFFFFFFFFFFFFFF, index, weight, count, rank, key))

    def replay_update_prios_dev(self, rp, index, prio, m):
        """prio[index[j]] = prio_new[j] for the m indices inside [0, max_size)"""
        self._check(self.lib.tetris_replay_update_prios_dev(self._h, C.byref(rp) if rp is not None else None, index, prio, int(m)))

    def replay_gather_dev(self, rp, index, m, steps, out):
        """The k-step views of index int32 [m] into out = traj_batch(...) sized for m * steps samples (sample j * steps + s =
        ring position index[j] + s; mirrored where the entry's flag says so)."""
        self._check(self.lib.tetris_replay_gather_dev(self._h, C.byref(rp) if rp is not None else None, index, int(m), int(steps),
                                                      C.byref(out) if out is not None else None))

    def replay_gather_steps_dev(self, rp, index, m, step_mask, out):
        """The rows of step_mask's bits (kstep_mask(steps); bit s: ring position index[j] + s) of the k-step views of index int32
        [m] into out = traj_batch(...) sized for m * n samples, n the number of bits: sample j * n + i = the i-th step."""
        self._check(self.lib.tetris_replay_gather_steps_dev(self._h, C.byref(rp) if rp is not None else None, index, int(m),
                                                            int(step_mask) & 0xFFFFFFFFFFFFFFFF, C.byref(out) if out is not None else None))

    # -- k-step target estimator (include/tetris_hip.h: tetris_kstep_target_dev)
    def kstep_target(self, out, reward, done, target, m, k_step, steps=None, index=None, max_size=0, values_mode=False, n_pieces=7,
                     n_values=1, used_pieces=None, f16=False, truncate=False, gamma=0.99, lam=0.9, values=None, done_time=None, step_mask=None,
                     mode=None, flags=0):
        """The argument struct of kstep_target_dev over raw DEVICE addresses or None: out = Q [m][n][4][10][n_pieces] (values_mode:
        v [m][n][n_values]) float32 (f16: binary16) for the n steps of `steps` (None: 1..k_step); ring mode: reward float32 / done
        uint8 = the ring's arrays with index int32 [m] and max_size; array mode (index None, max_size 0): reward / done [m][k_step +
        1]; target float32 [m], values float32 [m][n], done_time uint8 [m]."""
        val = lambda a: a.value if isinstance(a, C.c_void_p) else a               # noqa: E731
        t = KstepTarget()
        t.d_out, t.d_reward, t.d_done, t.d_index = val(out), val(reward), val(done), val(index)
        t.M, t.k_step, t.max_size = int(m), int(k_step), int(max_size)
        t.step_mask = int(step_mask) if step_mask is not None else kstep_mask(kstep_steps(k_step) if steps is None else steps)
        t.mode = int(mode) if mode is not None else (KSTEP_V if values_mode else KSTEP_Q)
        t.n_pieces, t.n_values = int(n_pieces), int(n_values)
        t.used_pieces = (1 << int(n_pieces)) - 1 if used_pieces is None else int(used_pieces)
        t.flags = (LOSS_F16 if f16 else 0) | (KSTEP_TRUNCATE if truncate else 0) | int(flags)
        t.gamma, t.lam = float(gamma), float(lam)
        t.d_target, t.d_values, t.d_done_time = val(target), val(values), val(done_time)
        return t

    def kstep_target_dev(self, t):
        """The k-step targets of a minibatch from the reference net's outputs for its step rows (t = kstep_target(...))."""
        self._check(self.lib.tetris_kstep_target_dev(self._h, C.byref(t) if t is not None else None))

    # -- output heads (include/tetris_hip.h: tetris_q_head_dev, tetris_policy_head_dev and their _grad_dev)
    def used_pieces(self, n_pieces=7):
        """The used_pieces mask of the batch's piece set (create_used_pieces_mask): bit p for every piece the games deal; 1 for a
        net with one piece plane."""
        if int(n_pieces) == 1:
            return 1
        mask = 0
        for p in self.piece_map:
            mask |= 1 << int(p)
        return mask

    def q_head(self, a, m, v=None, n_pieces=7, n_values=1, mode="mean", advantage_range=1.0, separate_piece_values=True, used_pieces=None,
               f16=False, value_f16=False, Q=None, V=None, A=None, grad_Q=None, grad_a=None, grad_v=None, flags=0):
        """The argument struct of q_head_dev / q_head_grad_dev over raw DEVICE addresses or None: a, Q, A, grad_Q, grad_a
        [m][4][10][n_pieces] float32 (f16: binary16), v, grad_v [m][n_values] float32 (value_f16: binary16) or None, V float32 [m].
        mode: "mean", "max", any other string (no normalisation) or a TETRIS_HEAD_* number; used_pieces None: the batch's piece set."""
        val = lambda x: x.value if isinstance(x, C.c_void_p) else x               # noqa: E731
        h = QHead()
        h.d_a, h.d_v, h.d_grad_Q = val(a), val(v), val(grad_Q)
        h.M, h.n_pieces, h.n_values = int(m), int(n_pieces), int(n_values)
        h.mode = HEAD_MODES.get(mode, HEAD_NONE) if isinstance(mode, str) else int(mode)
        h.separate_piece_values = 1 if separate_piece_values else 0
        h.used_pieces = self.used_pieces(n_pieces) if used_pieces is None else int(used_pieces)
        h.flags = (HEAD_F16 if f16 else 0) | (HEAD_VALUE_F16 if value_f16 else 0) | int(flags)
        h.advantage_range = float(advantage_range)
        h.d_Q, h.d_V, h.d_A, h.d_grad_a, h.d_grad_v = val(Q), val(V), val(A), val(grad_a), val(grad_v)
        return h

    def q_head_dev(self, h):
        """Q, V and (where given) A of a minibatch from the raw streams a and v (h = q_head(...))."""
        self._check(self.lib.tetris_q_head_dev(self._h, C.byref(h) if h is not None else None))

    def q_head_grad_dev(self, h):
        """grad_a and grad_v from grad_Q (h = q_head(...))."""
        self._check(self.lib.tetris_q_head_grad_dev(self._h, C.byref(h) if h is not None else None))

    def policy_head(self, m, pi, v, n_pieces=7, n_values=1, x=None, w=None, grad_pi=None, grad_v=None, grad_x=None, grad_w=None, f16=False,
                    value_f16=False, flags=0):
        """The argument struct of policy_head_dev / policy_head_grad_dev over raw DEVICE addresses or None: x, pi, grad_pi, grad_x
        [m][4][10][n_pieces] float32 (f16: binary16); w, grad_w [m][n_values], n_values = 1 or n_pieces + 1, and v, grad_v
        [m][1 or n_pieces] float32 (value_f16: binary16)."""
        val = lambda a: a.value if isinstance(a, C.c_void_p) else a               # noqa: E731
        h = PolicyHead()
        h.d_x, h.d_w, h.d_grad_pi, h.d_grad_v = val(x), val(w), val(grad_pi), val(grad_v)
        h.M, h.n_pieces, h.n_values = int(m), int(n_pieces), int(n_values)
        h.flags = (HEAD_F16 if f16 else 0) | (HEAD_VALUE_F16 if value_f16 else 0) | int(flags)
        h.d_pi, h.d_v, h.d_grad_x, h.d_grad_w = val(pi), val(v), val(grad_x), val(grad_w)
        return h

    def policy_head_dev(self, h):
        """pi and v of a minibatch from the logits x and the value stream w (h = policy_head(...))."""
        self._check(self.lib.tetris_policy_head_dev(self._h, C.byref(h) if h is not None else None))

    def policy_head_grad_dev(self, h):
        """grad_x and grad_w from the stored pi, v and grad_pi, grad_v (h = policy_head(...))."""
        self._check(self.lib.tetris_policy_head_grad_dev(self._h, C.byref(h) if h is not None else None))

    # -- network inputs (include/tetris_hip.h: tetris_net_input_dev)
    def net_input(self, m, obs=None, replay=None, index=None, row=0, steps=1, step_mask=0, items=("cumsum", "shadow", "height", "holes"), pad=True,
                  f16=False, channels_last=False, visual=None, vector=None, piece=None, valid=None, flags=0):
        """The argument struct of net_input_dev over raw DEVICE addresses or None.  The source is obs = traj_obs(...) with index int32
        [m] (bit 31: mirrored; out of range: no sample) or with index None and a row (m = n_games), or replay = replay(...) with
        index int32 [m] and steps (a count) or step_mask (kstep_mask(steps)): m * n samples.  items: names or TETRIS_INPUT_* codes in
        channel order.  Outputs: visual [S][m][C][Hp][Wp] (channels_last: [S][m][Hp][Wp][C]) and vector [S][m][12] float32 (f16:
        binary16), piece uint8 [S][m], valid uint8 [m]; (C, Hp, Wp) = input_shape(height, len(items), pad).  The struct keeps obs /
        replay alive."""
        val = lambda a: a.value if isinstance(a, C.c_void_p) else a               # noqa: E731
        n = NetInput()
        n._keep = (obs, replay)
        n.obs = C.addressof(obs) if obs is not None else None
        n.replay = C.addressof(replay) if replay is not None else None
        n.d_index, n.row, n.M, n.steps, n.step_mask = val(index), int(row), int(m), int(steps), int(step_mask) & 0xFFFFFFFFFFFFFFFF
        codes = [INPUT_ITEMS[i] if isinstance(i, str) else int(i) for i in items]
        n.n_items = len(codes)
        for i, code in enumerate(codes[:4]):
            n.items[i] = code
        n.flags = (INPUT_F16 if f16 else 0) | (INPUT_CHANNELS_LAST if channels_last else 0) | (INPUT_PAD if pad else 0) | int(flags)
        n.d_visual, n.d_vector, n.d_piece, n.d_valid = val(visual), val(vector), val(piece), val(valid)
        return n

    def net_input_dev(self, n):
        """The padded plane stack, the float vector, piece and valid of a set of samples straight from their packed records
        (n = net_input(...))."""
        self._check(self.lib.tetris_net_input_dev(self._h, C.byref(n) if n is not None else None))

    # -- keyboard convolution (include/tetris_hip.h: tetris_kbd_conv_dev, _grad_x_dev, _grad_w_dev)
    def kbd_conv(self, m, height, channels, n_pieces=7, x=None, w=None, bias=None, grad_out=None, out=None, grad_x=None, grad_w=None,
                 grad_b=None, f16=False, flags=0):
        """The argument struct of the three kbd_conv calls over raw DEVICE addresses or None: x, grad_x [m][height][12][channels],
        w [height][3][channels][4 n_pieces], out, grad_out [m][4][10][n_pieces] float32 (f16: binary16); bias, grad_b float32
        [4 n_pieces]; grad_w float32 like w."""
        val = lambda a: a.value if isinstance(a, C.c_void_p) else a               # noqa: E731
        k = KbdConv()
        k.d_x, k.d_w, k.d_bias, k.d_grad_out = val(x), val(w), val(bias), val(grad_out)
        k.M, k.n_pieces, k.height, k.channels = int(m), int(n_pieces), int(height), int(channels)
        k.flags = (KBD_F16 if f16 else 0) | int(flags)
        k.d_out, k.d_grad_x, k.d_grad_w, k.d_grad_b = val(out), val(grad_x), val(grad_w), val(grad_b)
        return k

    def kbd_conv_dev(self, k):
        """out = keyboard_conv(x) of a minibatch (k = kbd_conv(...))."""
        self._check(self.lib.tetris_kbd_conv_dev(self._h, C.byref(k) if k is not None else None))

    def kbd_conv_grad_x_dev(self, k):
        """grad_x from grad_out and w (k = kbd_conv(...))."""
        self._check(self.lib.tetris_kbd_conv_grad_x_dev(self._h, C.byref(k) if k is not None else None))

    def kbd_conv_grad_w_dev(self, k):
        """grad_w and grad_b from x and grad_out (k = kbd_conv(...))."""
        self._check(self.lib.tetris_kbd_conv_grad_w_dev(self._h, C.byref(k) if k is not None else None))

    # -- residual layer (include/tetris_hip.h: tetris_res_layer_dev, _grad_x_dev, _grad_w_dev)
    def res_layer(self, m, height, in_channels, out_channels, join="add", activation="elu", x=None, w=None, bias=None, y=None,
                  grad_out=None, out=None, grad_x=None, grad_w=None, grad_b=None, f16=False, flags=0):
        """The argument struct of the three res_layer calls over raw DEVICE addresses or None: x, grad_x [m][height][12][in_channels],
        w [3][3][in_channels][out_channels], out, y, grad_out [m][height][12][res_out_channels(...)] float32 (f16: binary16); bias,
        grad_b float32 [out_channels]; grad_w float32 like w.  join "none" / "add" / "truncate_add" and activation "none" / "elu"
        (or None, or the header's numbers)."""
        val = lambda a: a.value if isinstance(a, C.c_void_p) else a               # noqa: E731
        r = ResLayer()
        r.d_x, r.d_w, r.d_bias, r.d_y, r.d_grad_out = val(x), val(w), val(bias), val(y), val(grad_out)
        r.M, r.height, r.in_channels, r.out_channels = int(m), int(height), int(in_channels), int(out_channels)
        r.join, r.activation = int(RES_JOINS.get(join, join)), int(RES_ACTS.get(activation, activation))
        r.flags = (RES_F16 if f16 else 0) | int(flags)
        r.d_out, r.d_grad_x, r.d_grad_w, r.d_grad_b = val(out), val(grad_x), val(grad_w), val(grad_b)
        return r

    def res_layer_dev(self, r):
        """out = act(join(x, conv3x3(x))) of a minibatch (r = res_layer(...))."""
        self._check(self.lib.tetris_res_layer_dev(self._h, C.byref(r) if r is not None else None))

    def res_layer_grad_x_dev(self, r):
        """grad_x from grad_out, w and, with ELU, y (r = res_layer(...))."""
        self._check(self.lib.tetris_res_layer_grad_x_dev(self._h, C.byref(r) if r is not None else None))

    def res_layer_grad_w_dev(self, r):
        """grad_w and grad_b from x, grad_out and, with ELU, y (r = res_layer(...))."""
        self._check(self.lib.tetris_res_layer_grad_w_dev(self._h, C.byref(r) if r is not None else None))

    # -- loss heads (include/tetris_hip.h: tetris_ppo_loss_dev, tetris_dqn_loss_dev)
    def ppo_loss(self, pi, v, action, prob_old, adv, target, grad_pi, grad_v, stats, m, n_pieces=7, n_values=1, valid=None, terms=None,
                 f16=False, value_f16=False, grad_f16=False, clipping_parameter=0.15, value_loss=1.0, policy_loss=1.0, entropy_loss=0.0,
                 ppo_epsilon=None, entropy_floor_loss=0.0, rescaled_entropy=0.0, entropy_floor=None, grad_scale=1.0, flags=0):
        """The argument struct of ppo_loss_dev over raw DEVICE addresses (int / c_void_p) or None: pi, grad_pi [m][4][10][n_pieces]
        and v, grad_v [m][n_values] float32 (f16 / value_f16 / grad_f16: binary16), action uint8 [m][3], prob_old / adv / target
        float32 [m], valid uint8 [m], terms float32 [6][m], stats float32 [16].  The parameter names are model.train's; the
        floor comes from ppo_epsilon (ppo_entropy_constants) unless entropy_floor gives it."""
        val = lambda a: a.value if isinstance(a, C.c_void_p) else a               # noqa: E731
        l = PpoLoss()
        l.d_pi, l.d_v, l.d_action, l.d_prob_old, l.d_adv, l.d_target = val(pi), val(v), val(action), val(prob_old), val(adv), val(target)
        l.d_valid, l.M, l.n_pieces, l.n_values = val(valid), int(m), int(n_pieces), int(n_values)
        l.flags = (LOSS_F16 if f16 else 0) | (LOSS_VALUE_F16 if value_f16 else 0) | (LOSS_GRAD_F16 if grad_f16 else 0) | int(flags)
        l.clip, l.value_loss, l.policy_loss, l.entropy_loss = float(clipping_parameter), float(value_loss), float(policy_loss), float(entropy_loss)
        floor, hmax = ppo_entropy_constants(0.0 if ppo_epsilon is None else ppo_epsilon)
        l.entropy_floor_loss, l.rescaled_entropy = float(entropy_floor_loss), float(rescaled_entropy)
        l.entropy_floor, l.max_entropy = float(floor if entropy_floor is None else entropy_floor), hmax
        l.grad_scale, l.reserved = float(grad_scale), 0.0
        l.d_grad_pi, l.d_grad_v, l.d_terms, l.d_stats = val(grad_pi), val(grad_v), val(terms), val(stats)
        return l

    def ppo_loss_dev(self, l):
        """The PPO loss of a minibatch, its statistics and its gradient with respect to pi and v (l = ppo_loss(...))."""
        self._check(self.lib.tetris_ppo_loss_dev(self._h, C.byref(l) if l is not None else None))

    def dqn_loss(self, Q, action, target, grad_Q, new_prio, stats, m, n_pieces=7, weight=None, valid=None, q=None, f16=False, grad_f16=False,
                 optimistic_prios=0.0, grad_scale=1.0, flags=0):
        """The argument struct of dqn_loss_dev over raw DEVICE addresses or None: Q, grad_Q [m][4][10][n_pieces] float32 (f16 /
        grad_f16: binary16), action uint8 [m][3], target / weight / new_prio / q float32 [m], valid uint8 [m], stats float32 [16]."""
        val = lambda a: a.value if isinstance(a, C.c_void_p) else a               # noqa: E731
        l = DqnLoss()
        l.d_Q, l.d_action, l.d_target, l.d_weight, l.d_valid = val(Q), val(action), val(target), val(weight), val(valid)
        l.M, l.n_pieces = int(m), int(n_pieces)
        l.flags = (LOSS_F16 if f16 else 0) | (LOSS_GRAD_F16 if grad_f16 else 0) | int(flags)
        l.optimistic_prios, l.grad_scale, l.reserved = float(optimistic_prios), float(grad_scale), 0.0
        l.d_grad_Q, l.d_new_prio, l.d_q, l.d_stats = val(grad_Q), val(new_prio), val(q), val(stats)
        return l

    def dqn_loss_dev(self, l):
        """The DQN loss of a minibatch, its statistics, its gradient with respect to Q and the samples' new priorities
        (l = dqn_loss(...))."""
        self._check(self.lib.tetris_dqn_loss_dev(self._h, C.byref(l) if l is not None else None))

    def plan_loss(self, phi, v, index, piece, prob_old, adv, target, grad_phi, grad_v, stats, m, n_pieces=7, n_values=1, piece_stride=1,
                  valid=None, terms=None, f16=False, value_f16=False, grad_f16=False, small_fill=0.0, clipping_parameter=0.15, value_loss=1.0,
                  policy_loss=1.0, entropy_loss=0.0, impossibility_loss=0.0, grad_scale=1.0, flags=0):
        """The argument struct of plan_loss_dev over raw DEVICE addresses (int / c_void_p) or None: phi, grad_phi [m][H][10][n_pieces]
        and v, grad_v [m][n_values] float32 (f16 / value_f16 / grad_f16: binary16), index int32 [m] (entries of the planning window;
        bit 31: mirrored), piece uint8 with sample j's piece at byte j * piece_stride (1: a uint8 [m] array; 3: the address of
        byte 2 of a batch's action [m][3]), prob_old / adv / target float32 [m], valid uint8 [m], terms float32 [6][m], stats
        float32 [16].  The parameter names are model.train's; small_fill as traj_plan_batch_dev's (0: the reference's planes)."""
        val = lambda a: a.value if isinstance(a, C.c_void_p) else a               # noqa: E731
        l = PlanLoss()
        l.d_phi, l.d_v, l.d_index, l.d_piece = val(phi), val(v), val(index), val(piece)
        l.d_prob_old, l.d_adv, l.d_target, l.d_valid = val(prob_old), val(adv), val(target), val(valid)
        l.M, l.n_pieces, l.n_values, l.piece_stride = int(m), int(n_pieces), int(n_values), int(piece_stride)
        l.flags = (LOSS_F16 if f16 else 0) | (LOSS_VALUE_F16 if value_f16 else 0) | (LOSS_GRAD_F16 if grad_f16 else 0) | int(flags)
        l.small_fill, l.clip = float(small_fill), float(clipping_parameter)
        l.value_loss, l.policy_loss, l.entropy_loss, l.impossibility_loss = float(value_loss), float(policy_loss), float(entropy_loss), float(impossibility_loss)
        l.grad_scale = float(grad_scale)
        l.d_grad_phi, l.d_grad_v, l.d_terms, l.d_stats = val(grad_phi), val(grad_v), val(terms), val(stats)
        return l

    def plan_loss_dev(self, plan, l):
        """The planning agent's PPO loss of a minibatch straight from the plan records (plan = traj_plan(...), l = plan_loss(...)):
        its statistics and its gradient with respect to phi and v."""
        ref = lambda s: C.byref(s) if s is not None else None                     # noqa: E731
        self._check(self.lib.tetris_plan_loss_dev(self._h, ref(plan), ref(l)))

    def rollout_game_totals_dev(self, totals):
        """The per-game words rollout_totals sums: totals uint32 [4][N] = env-steps, episodes, lines cleared, garbage lines sent."""
        self._check(self.lib.tetris_rollout_game_totals_dev(self._h, totals))

    def rollout_random(self, launches, steps_per_launch=1, policy_seed=0xD71, first_step=0, ms=400):
        """-> (counters[4] = env_steps, episodes, lines, sent; elapsed_ms on the batch's stream)"""
        counters = np.zeros(4, np.uint64)
        elapsed = C.c_float(0.0)
        self._check(self.lib.tetris_rollout_random(self._h, int(launches), int(steps_per_launch), int(policy_seed), int(first_step),
                                                   int(ms), _p(counters), C.byref(elapsed)))
        return counters, float(elapsed.value)

    @staticmethod
    def split_words(my_a=None, opp_a=None, b0=None, b1=None):
        """The four exchange-word buffers of a split-mode step as the C array the stage calls take: raw device addresses
        (int) of uint32 [n] — my A words, the opponent's A words, player 0's B words, player 1's B words — or None."""
        return (C.c_void_p * 4)(*[C.c_void_p(int(p)) if p else C.c_void_p(0) for p in (my_a, opp_a, b0, b1)])

    def split_stage(self, stage, rot=None, trans=None, acting=None, words=None, out=None, done=None, lines=None, dead=None, ms=400):
        """One stage of a split-mode step; `words` = split_words(...), every other argument a raw device address (int) or None."""
        self._check(self.lib.tetris_split_stage_dev(self._h, int(stage), rot, trans, acting, int(ms), words, out, done, lines, dead))

    def split_rollout_stage(self, stage, step, words=None, out=None, policy_seed=0xD71, ms=400):
        self._check(self.lib.tetris_split_rollout_stage_dev(self._h, int(stage), int(policy_seed), int(step), int(ms), words, out))

    def rollout_launch(self, launches, steps_per_launch=1, policy_seed=0xD71, first_step=0, ms=400):
        """The launches of rollout_random alone (what bench.py times).  -> elapsed_ms between HIP events around them."""
        elapsed = C.c_float(0.0)
        self._check(self.lib.tetris_rollout_launch(self._h, int(launches), int(steps_per_launch), int(policy_seed), int(first_step),
                                                   int(ms), C.byref(elapsed)))
        return float(elapsed.value)

    def rollout_totals(self):
        """-> uint64 [4]: cumulative env-steps (counted on the device), episodes, lines cleared, garbage lines sent of this
        batch's built-in rollouts."""
        t = np.zeros(4, np.uint64)
        self._check(self.lib.tetris_rollout_totals(self._h, _p(t)))
        return t

    def set_stream(self, stream_ptr, external=True):
        """Run on a caller-owned HIP stream (handle as int; 0 = the legacy default stream).  external=False: own stream."""
        self._check(self.lib.tetris_set_stream(self._h, C.c_void_p(int(stream_ptr) if stream_ptr else 0), 1 if external else 0))

    def set_chained(self, on):
        """Chained launches of the built-in rollout on / off (include/tetris_hip.h: tetris_set_chained)."""
        self._check(self.lib.tetris_set_chained(self._h, 1 if on else 0))

    def set_direct_dispatch(self, on, min_launches=None):
        """Long chained calls through HSA queues of the library's own (AQL packets written by the library) on / off;
        min_launches: calls of at least that many launches (default: the library's, 16) — include/tetris_hip.h:
        tetris_set_direct_dispatch."""
        self._check(self.lib.tetris_set_direct_dispatch(self._h, 0 if not on else (-1 if min_launches is None else max(1, int(min_launches)))))

    def rollout_was_direct(self):
        rc = self.lib.tetris_rollout_was_direct(self._h)
        if rc < 0:
            self._check(rc)
        return bool(rc)

    def rollout_was_affine(self):
        """The last rollout call ran the XCD-affine chained kernel (include/tetris_hip.h: tetris_set_xcd_affine)."""
        rc = self.lib.tetris_rollout_was_direct(self._h)
        if rc < 0:
            self._check(rc)
        return rc == 2

    def set_xcd_affine(self, on):
        self._check(self.lib.tetris_set_xcd_affine(self._h, 1 if on else 0))

    def debug_xcd_skew(self, skew):
        """Test aid: the kernels are told start XCDs that are off by `skew` (every workgroup then finds itself misplaced)."""
        self._check(self.lib.tetris_debug_xcd_skew(self._h, int(skew)))

    def debug_table_limit(self, chunks):
        """Test aid (include/tetris_hip.h: tetris_debug_table_limit): this batch's episodes end with TETRIS_ERR_STREAM after
        624 * chunks piece draws (1..64; 0 = the real limit, 64)."""
        self._check(self.lib.tetris_debug_table_limit(self._h, int(chunks)))

    def set_chain_spin_limit(self, polls):
        """Polls of the predecessor's epoch word after which a waiting wave of a chained launch gives up (0 = default, ~2 s)."""
        self._check(self.lib.tetris_set_chain_spin_limit(self._h, int(polls)))

    def debug_stall(self, which, microseconds, percent=0):
        """Test aid (include/tetris_hip.h: tetris_debug_stall): idle kernel on chain stream 0..2, on the batch's stream (3) or,
        which = -1, holding `percent` % of the device's wave slots on a stream of its own."""
        self._check(self.lib.tetris_debug_stall(self._h, int(which), int(microseconds), int(percent)))

    def debug_chain_epoch(self, epoch=None):
        """Test aid (include/tetris_hip.h: tetris_debug_chain_epoch): with `epoch`, the batch looks as if that many chained launches
        had already run (every wave's epoch word and the batch's count); -> the batch's count of chained launches afterwards."""
        out = C.c_uint32(0)
        self._check(self.lib.tetris_debug_chain_epoch(self._h, -1 if epoch is None else int(epoch), C.byref(out)))
        return int(out.value)

    def clock_mhz(self):
        """Measurement aid: the GPU's shader clock of the moment (tetris_debug_clock_khz)."""
        khz = C.c_int(0)
        self._check(self.lib.tetris_debug_clock_khz(self._h, C.byref(khz)))
        return khz.value / 1000.0

    def rollout_is_chained(self, steps_per_launch=1):
        rc = self.lib.tetris_rollout_is_chained(self._h, int(steps_per_launch))
        if rc < 0:
            self._check(rc)
        return bool(rc)

    def set_game_offset(self, first_game_id):
        self._check(self.lib.tetris_set_game_offset(self._h, int(first_game_id)))

    def timer_start(self):
        self._check(self.lib.tetris_timer_start(self._h))

    def timer_stop(self):
        ms = C.c_float(0.0)
        self._check(self.lib.tetris_timer_stop(self._h, C.byref(ms)))
        return float(ms.value)

    def sync(self):
        self._check(self.lib.tetris_sync(self._h))

    def take_errors(self):
        """-> TETRIS_ERR_* bits since the last call: 1 = a garbage queue overflowed, 2 = an episode outran the RNG tables (games
        ended by a capacity error; which games: observe()[0]["fifo_overflow"]); 4 = a chained rollout call fell back to
        un-chained launches for some games (results unaffected, chaining is now off for this batch); 8 = some game's key lists did
        not fit the buffers of action_lists_dev (its count is -1)."""
        bits = C.c_uint32(0)
        self._check(self.lib.tetris_take_errors(self._h, C.byref(bits)))
        return int(bits.value)

    @property
    def table_chunks(self):
        return self.lib.tetris_table_chunks(self._h)
