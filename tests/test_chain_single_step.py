"""The chained rollout kernels by step count.  A chained call of one step per launch runs the single-step kernels (k_chain<1>,
k_chain_affine<1>: rollout_step once, no loop), any other step count the fused ones (k_chain_fused<1>, k_chain_fused_affine<1>:
game_run's loop).  Both share rollout_step (csrc/tetris_kernels.h), so K launches of one step, one launch of K steps and the
oracle (PythonHandle.cpp:149-188 per step) must leave the same boards and counters — on the CPU harness, which compiles the
same bodies, and on the GPU through every launch path, with the step counts taking turns on one batch."""
import os

import numpy as np
import pytest

from oracle import oracle as orc
from tests import engines

THREADS = min(32, len(os.sched_getaffinity(0)))


def _same(eng, ref, n, where=""):
    for lo in range(0, n, 8192):
        idx = np.arange(lo, min(n, lo + 8192), dtype=np.int32)
        engines.assert_same_state(eng, ref, idx=idx, where=f"{where} games {lo}..")


@pytest.mark.parametrize("P,K", [(1, 1), (1, 37), (1, 120), (2, 48)])
def test_cpu_k_launches_of_one_step_equal_one_launch_of_k_steps(P, K):
    """CPU harness: K launches of S = 1 against one launch of S = K against the oracle, state and counters; then the same
    again from where that left the boards (a first_step other than 0), with a launch of no steps in between."""
    n = 192
    seeds = orc.episode_seed(np.arange(n), 0)
    single, fused = engines.make("harness", n, P, seeds=seeds), engines.make("harness", n, P, seeds=seeds)
    ref = engines.make("oracle", n, P, seeds=seeds)
    step, ep = 0, None                # (the oracle keeps no episode numbers: its caller carries them from call to call)
    for rep in range(2):
        c1, _ = single.rollout_random(K, 1, first_step=step)
        cK, _ = fused.rollout_random(1, K, first_step=step)
        ep, want = ref.rollout_random(K, first_step=step, episode=ep)
        assert c1.tolist() == cK.tolist() == want.tolist()
        assert int(c1[0]) == n * K
        engines.assert_same_state(single, ref, where=f"K launches of one step, round {rep}")
        engines.assert_same_state(fused, ref, where=f"one launch of K steps, round {rep}")
        step += K
        c0, _ = single.rollout_random(2, 0, first_step=step)
        assert c0.tolist() == [0, 0, 0, 0]
        engines.assert_same_state(single, ref, where=f"launches of no steps, round {rep}")


# (launches, steps per launch) of consecutive chained calls: S = 1, S = 3 and S = 0 take turns, in calls long and short
TURNS = [(20, 1), (6, 3), (17, 0), (33, 1), (16, 3), (1, 1), (2, 0), (5, 3), (40, 1), (18, 0), (7, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["queues_affine", "queues_write_through", "streams"])
def test_gpu_step_counts_take_turns_bit_exact(path):
    """One 65 536-board batch, chained calls with S = 1, S = 3 and S = 0 taking turns, against the oracle bit for bit: through the
    library's queues with the XCD-affine kernels, through the queues with tetris_set_xcd_affine(b, 0), and through the streams
    (calls of fewer than 16 launches)."""
    n = 65536
    seeds = orc.episode_seed(np.arange(n), 0)
    eng, ref = engines.make("hip", n, 1, seeds=seeds), engines.make("oracle", n, 1, seeds=seeds)
    for S in (0, 1, 3):
        assert eng.rollout_is_chained(S)
    if path == "queues_write_through":
        eng.set_xcd_affine(False)
    if path != "streams":
        eng.set_direct_dispatch(True, min_launches=1)
    total, step = np.zeros(4, np.uint64), 0
    for launches, S in TURNS:
        if path == "streams":
            launches = min(launches, 15)
        c, _ = eng.rollout_random(launches, S, first_step=step)
        assert eng.rollout_was_direct() == (path != "streams")
        if path == "queues_affine":
            assert eng.rollout_was_affine()
        assert int(c[0]) == n * launches * S
        total += c
        step += launches * S
    _, want = ref.rollout_random(step, threads=THREADS)
    assert total.tolist() == want.tolist()
    _same(eng, ref, n, where=path)
    assert eng.take_errors() == 0
    for S in (0, 1, 3):
        assert eng.rollout_is_chained(S)                    # no wave gave up, nothing fell back
