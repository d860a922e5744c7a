#!/usr/bin/env python3
"""CONTAINER-ONLY fixture generator: what the reference's planning trajectory returns for seeded episodes.

Loads the reference's own `agents/datatypes/trajectory.py` the way make_traj_golden.py does, fills a `sherlock_trajectory` per
episode through its own `add` with the seven-tuple sherlock_agent.get_action stores per step (sherlock_agent.py:137-146), in that
tuple's shapes — a_idx, piece, pi(a), v_piece, v_mean [1, 1] each, delta(s, a) and delta_sum(s) [1, H, 10, 1] — and runs
`process_trajectory(compute_advantages=True)`.

The fields are this script's own: per entry a random stack `before` and L = 5 afterstates `after` — four cells more (a whole
piece), three cells more (the "fewer than 4 cells" rule), two cells gone and six more (a cleared-and-landed shape: negative
deltas), five cells more, and no change (the rule again).  delta and delta_sum are formed from them by the rule of
sherlock_utils.deltas / generate_deltas as include/tetris_hip.h states it with small_fill = 0 (the reference's uint8 fields turn
its 1e-3 into 0): after - before per list, a list whose difference adds up to less than 4 is zero everywhere, delta_sum = the
sum over the lists.  Episode lengths 1, 2, 3 and 17; the reward is +1 or -1 on the last entry, which is also the only `done`;
values are float32 numbers drawn from 2 N(0, 1); (gamma, gae_lambda) is (0.98, 0.96) and (-0.98, 0.7); H = 20.

Nothing of the reference is copied: tests/golden/traj_plan.npz holds inputs and the returned arrays only, all episodes of all
cases laid end to end:
    case [E] index into gamma / gae_lambda, start [E], length [E]
    before bool [sum, H, 10], after bool [sum, L, H, 10]                                       the inputs
    a_idx, piece int64 [sum], prob, v_piece, v_mean, reward float32 [sum], done uint8 [sum]
    out0 .. out6 float64                         the seven arrays of the returned `a`, in its order: a_idx, piece, prob, adv,
                                                 target [sum, 1], delta, delta_sum [sum, H, 10, 1]
    r float64 [sum, 1], d uint8 [sum, 1]         the returned reward and done
    gamma, gae_lambda float64 [2], gve_lambda float64 []
tests/test_traj_plan.py lays the episodes into one window and compares.
Run:  python tests/golden/make_traj_plan_golden.py        (needs /root/reference)
"""
import os

import numpy as np

from make_traj_golden import CASES, GVE_LAMBDA, import_trajectory

HERE = os.path.dirname(os.path.abspath(__file__))
LENGTHS = (1, 2, 3, 17)
H, L = 20, 5


def fields(rng, entry):
    """-> before bool [H, 10], after bool [L, H, 10]"""
    before = np.zeros((H, 10), bool)
    top = int(rng.integers(8, 15))                                   # rows top .. H-1 hold the stack (row 0 is the top row)
    before[top:] = rng.random((H - top, 10)) < 0.7
    before[top:, int(rng.integers(0, 10))] = False                   # no full rows
    after = np.repeat(before[None], L, axis=0)
    free, used = np.argwhere(~before), np.argwhere(before)
    for k in range(L):
        case = (entry + k) % 5
        more = {0: 4, 1: 3, 2: 6, 3: 5, 4: 0}[case]
        if case == 2:
            for y, x in used[rng.permutation(len(used))[:2]]:
                after[k, y, x] = False
        for y, x in free[rng.permutation(len(free))[:more]]:
            after[k, y, x] = True
    return before, after


def planes(before, after, a_idx):
    """-> delta float64 [1, H, 10, 1] of list a_idx, delta_sum float64 [1, H, 10, 1] (small_fill = 0)"""
    d = after.astype(np.float64) - before[None].astype(np.float64)          # [L, H, 10]
    d[d.sum(axis=(1, 2)) < 4.0] = 0.0
    return d[a_idx][None, :, :, None], d.sum(axis=0)[None, :, :, None]


def main():
    mod = import_trajectory()
    rng = np.random.default_rng(20261020)
    names = ("case", "start", "length", "before", "after", "a_idx", "piece", "prob", "v_piece", "v_mean", "reward", "done", "r", "d")
    out = {k: [] for k in names + tuple(f"out{j}" for j in range(7))}
    at = 0
    for case, (gamma, gae_lambda) in enumerate(CASES):
        for length in LENGTHS:
            v_piece = (2.0 * rng.standard_normal(length)).astype(np.float32)
            v_mean = (2.0 * rng.standard_normal(length)).astype(np.float32)
            prob = rng.random(length).astype(np.float32)
            a_idx, piece = rng.integers(0, L, length), rng.integers(0, 7, length)
            reward = np.zeros(length, np.float32)
            reward[-1] = 1.0 if rng.integers(0, 2) else -1.0
            done = np.zeros(length, np.uint8)
            done[-1] = 1
            tr = mod.sherlock_trajectory()
            before, after = [], []
            for t in range(length):
                bf, af = fields(rng, at + t)
                before.append(bf)
                after.append(af)
                delta, delta_sum = planes(bf, af, int(a_idx[t]))
                one = lambda v: np.array(v)[np.newaxis, np.newaxis]                                       # noqa: E731
                a = (one(int(a_idx[t])), one(int(piece[t])), one(float(prob[t])), one(float(v_piece[t])), one(float(v_mean[t])), delta, delta_sum)
                value = float(reward[t])
                tr.add((t, a, (lambda value=value: value), None, 0, bool(done[t])))
            data, _ = tr.process_trajectory(None, lambda s, player=None: s, compute_advantages=True, gamma_discount=gamma, gae_lambda=gae_lambda)
            _, a_out, r, d = data
            assert len(a_out) == 7 and np.array_equal(r[:, 0], reward) and np.array_equal(d[:, 0], done)
            for k, v in (("case", case), ("start", at), ("length", length)):
                out[k].append(v)
            for k, v in (("before", np.stack(before)), ("after", np.stack(after)), ("a_idx", a_idx), ("piece", piece), ("prob", prob),
                         ("v_piece", v_piece), ("v_mean", v_mean), ("reward", reward), ("done", done), ("r", np.asarray(r, np.float64)),
                         ("d", np.asarray(d, np.uint8))):
                out[k].append(v)
            for j in range(7):
                out[f"out{j}"].append(np.asarray(a_out[j], np.float64))
            at += length
    arrays = {k: np.asarray(out[k], np.int64) for k in ("case", "start", "length")}
    arrays.update({k: np.concatenate(v) for k, v in out.items() if k not in arrays})
    arrays.update(gamma=np.array([c[0] for c in CASES]), gae_lambda=np.array([c[1] for c in CASES]), gve_lambda=np.array(GVE_LAMBDA))
    path = os.path.join(HERE, "traj_plan.npz")
    np.savez_compressed(path, **arrays)
    print(f"{path}: {len(arrays['case'])} episodes, {at} entries, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
