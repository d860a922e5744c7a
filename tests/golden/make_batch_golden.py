#!/usr/bin/env python3
"""CONTAINER-ONLY fixture generator: the reference's augmented samples for seeded episodes.

Loads the reference's own `agents/datatypes/trajectory.py` from /root/reference the way make_traj_golden.py does, fills a
`sventon_trajectory` per episode through its own `add` and runs `process_trajectory(augment=True)`, which calls `augment_data`
(trajectory.py:88-109).  Episode lengths 1, 2 and 17.  The state of entry k is its TAG, a distinct number below 2^20; the
`state_fcn` stub returns ((vec, vec), (vis, vis), p) arrays that hold the tags, plus 2^20 when called with mirrored=True, so the
output shows which state, mirrored or not, the reference puts at every position.

Nothing of the reference is copied: tests/golden/traj_augment.npz holds inputs and outputs only, all episodes laid end to end:
    start [E], length [E]
    tag_in int64 [sum], a_env_in uint8 [sum, 3] (r, t, piece), prob float32 [sum], done_in uint8 [sum]      the inputs
    a_env_out uint8 [2 sum, 3], a_int_out float64 [2 sum, 3], r_out float64 [2 sum, 1], d_out uint8 [2 sum, 1]
    tag_out int64 [2 sum], tag_mirrored uint8 [2 sum]                                                   the state at each position
(an episode of length L owns positions 2 start .. 2 start + 2 L).  tests/test_traj_batch.py compares select + batch with it.
Run:  python tests/golden/make_batch_golden.py        (needs /root/reference)
"""
import os

import numpy as np

from make_traj_golden import import_trajectory

HERE = os.path.dirname(os.path.abspath(__file__))
LENGTHS = (1, 2, 17)
OFFSET = 1 << 20


def state_fcn(s, player=None, mirrored=False):
    t = np.asarray(s, np.int64).reshape(-1, 1) + (OFFSET if mirrored else 0)
    return [[t, t], [t, t], t]


def main():
    mod = import_trajectory()
    rng = np.random.default_rng(20261019)
    tags = rng.permutation(np.arange(1, OFFSET))[: sum(LENGTHS)]
    out = {k: [] for k in ("start", "length", "tag_in", "a_env_in", "prob", "done_in", "a_env_out", "a_int_out", "r_out", "d_out", "tag_out",
                           "tag_mirrored")}
    at = 0
    for length in LENGTHS:
        tag = tags[at:at + length]
        a_env = np.stack([rng.integers(0, 4, length), rng.integers(0, 10, length), rng.integers(0, 7, length)], axis=1).astype(np.uint8)
        if length == 17:
            a_env[:7, 2] = np.arange(7)                    # every piece and both ends of t are mirrored at least once
            a_env[:2, 1] = (0, 9)
        prob = rng.random(length).astype(np.float32)
        done = np.zeros(length, np.uint8)
        done[-1] = 1
        tr = mod.sventon_trajectory()
        for t in range(length):
            a_int = (float(prob[t]), 0.0, 0.0)
            value = 1.0 if done[t] else 0.0
            tr.add((int(tag[t]), (tuple(int(v) for v in a_env[t]), a_int), (lambda value=value: value), None, t % 2, bool(done[t])))
        data, _ = tr.process_trajectory(None, state_fcn, augment=True)
        S, (a_env_out, a_int_out), r, d = data
        states = np.asarray(S[1][0])[:, 0]
        assert all(np.array_equal(np.asarray(x)[:, 0], states) for x in (S[0][0], S[0][1], S[1][1], S[2]))
        for k, v in (("start", at), ("length", length)):
            out[k].append(v)
        for k, v in (("tag_in", tag), ("a_env_in", a_env), ("prob", prob), ("done_in", done), ("a_env_out", np.asarray(a_env_out, np.uint8)),
                     ("a_int_out", np.asarray(a_int_out, np.float64)), ("r_out", np.asarray(r, np.float64)), ("d_out", np.asarray(d, np.uint8)),
                     ("tag_out", states % OFFSET), ("tag_mirrored", (states // OFFSET).astype(np.uint8))):
            out[k].append(v)
        at += length
    arrays = {k: np.asarray(out[k], np.int64) for k in ("start", "length")}
    arrays.update({k: np.concatenate(out[k]) for k in out if k not in arrays})
    path = os.path.join(HERE, "traj_augment.npz")
    np.savez_compressed(path, **arrays)
    print(f"{path}: {len(LENGTHS)} episodes, {at} entries, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
