#!/usr/bin/env python3
"""CONTAINER-ONLY fixture generator: the reference's advantages and value targets for seeded episodes.

Loads the reference's own `agents/datatypes/trajectory.py` from /root/reference with a stub for `tools.utils` (the module
imports it and never uses it), fills a `sventon_trajectory` per episode through its own `add` and runs
`process_trajectory(compute_advantages=True)`, which calls `adv_and_targets` (trajectory.py:56-86, 111-141) with its default
gve_lambda = 0.95.  Episode lengths 1, 2, 3, 17, 64, 257 and 1 581; the reward is +1 or -1 on the last entry, which is also
the only `done`; values are float32 numbers drawn from 2 N(0, 1), handed to the reference as float64; (gamma, gae_lambda) is
(0.98, 0.96) and (-0.98, 0.7) (single-policy self-play negates gamma: sventon_agent_base.py:76).

Nothing of the reference is copied: tests/golden/traj_gae.npz holds inputs and float64 outputs only, all episodes of all cases
laid end to end:
    case [E] index into gamma / gae_lambda, start [E], length [E]
    v_piece, v_mean float32 [sum], reward float32 [sum], done uint8 [sum]          the inputs (a_internal[1], a_internal[2], r, d)
    adv, target float64 [sum]                                                      a_int_np[:, 1], a_int_np[:, 2]
    gamma, gae_lambda float64 [2], gve_lambda float64 []
tests/test_traj_device.py lays the episodes into one window and compares.
Run:  python tests/golden/make_traj_golden.py        (needs /root/reference)
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
LENGTHS = (1, 2, 3, 17, 64, 257, 1581)
CASES = ((0.98, 0.96), (-0.98, 0.7))
GVE_LAMBDA = 0.95


def import_trajectory():
    if not os.path.isdir(REF):
        raise SystemExit("/root/reference is not present: fixtures can only be generated in the build container")
    tools = types.ModuleType("tools")
    tools.utils = types.ModuleType("tools.utils")
    sys.modules.setdefault("tools", tools)
    sys.modules.setdefault("tools.utils", tools.utils)
    spec = importlib.util.spec_from_file_location("ref_trajectory", os.path.join(REF, "agents", "datatypes", "trajectory.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    mod = import_trajectory()
    rng = np.random.default_rng(20261018)
    out = {k: [] for k in ("case", "start", "length", "v_piece", "v_mean", "reward", "done", "adv", "target")}
    at = 0
    for case, (gamma, gae_lambda) in enumerate(CASES):
        for length in LENGTHS:
            v_piece = (2.0 * rng.standard_normal(length)).astype(np.float32)
            v_mean = (2.0 * rng.standard_normal(length)).astype(np.float32)
            reward = np.zeros(length, np.float32)
            reward[-1] = 1.0 if rng.integers(0, 2) else -1.0
            done = np.zeros(length, np.uint8)
            done[-1] = 1
            tr = mod.sventon_trajectory()
            for t in range(length):
                a_env = (int(rng.integers(0, 4)), int(rng.integers(0, 10)), int(rng.integers(0, 7)))
                a_int = (float(rng.random()), float(v_piece[t]), float(v_mean[t]))
                value = float(reward[t])
                tr.add((t, (a_env, a_int), (lambda value=value: value), None, t % 2, bool(done[t])))
            data, _ = tr.process_trajectory(None, lambda s, player=None: s, compute_advantages=True, gamma_discount=gamma,
                                            gae_lambda=gae_lambda)
            _, (a_env_np, a_int_np), r, d = data
            assert np.array_equal(r[:, 0], reward) and np.array_equal(d[:, 0], done) and a_int_np.dtype == np.float64
            for k, v in (("case", case), ("start", at), ("length", length)):
                out[k].append(v)
            for k, v in (("v_piece", v_piece), ("v_mean", v_mean), ("reward", reward), ("done", done), ("adv", a_int_np[:, 1]),
                         ("target", a_int_np[:, 2])):
                out[k].append(v)
            at += length
    arrays = {k: np.asarray(out[k], np.int64) for k in ("case", "start", "length")}
    arrays.update({k: np.concatenate(out[k]) for k in ("v_piece", "v_mean", "reward", "done", "adv", "target")})
    arrays.update(gamma=np.array([c[0] for c in CASES]), gae_lambda=np.array([c[1] for c in CASES]), gve_lambda=np.array(GVE_LAMBDA))
    path = os.path.join(HERE, "traj_gae.npz")
    np.savez_compressed(path, **arrays)
    print(f"{path}: {len(arrays['case'])} episodes, {at} entries, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
