#!/usr/bin/env python3
"""CONTAINER-ONLY fixture generator: the reference's experience replay as a ring, ranked and sampled.

Loads the reference's own `agents/agent_utils/experience_replay.py` and `fcns.py` from /root/reference by path, under a stub
`agents.agent_utils` package that holds nothing but their `k_step_view`, builds `experience_replay(max_size=40, k_step=3)` with
one vector and one visual state of one number each — the state of an entry is its TAG, the running number of the entry, 1 for
the first — and calls `add_samples` with 11, 17, 9, 12, 30 and 5 entries.  Then it ranks and samples a priority
vector with a block of equal values, a 0.0 and a -0.0 through `get_random_sample(n_samples=n, alpha=0.7, beta=0.6)` and runs one
`update_prios`.

Nothing of the reference is copied: tests/golden/replay_ring.npz holds inputs and outputs only:
    max_size, k_step, adds [6]                      the set-up
    slice_start [6], slice_stop [6]                 the slice add_indices returned for each add
    cursor int64 [6, 2]                             (current_idx, current_size) after each add
    ring int64 [40]                                 the final _visual_states[0] (tags; rows 37..39 were never written)
    done uint8 [40], reward float32 [40], action float32 [40, 3]
    view_at int64 [3], view int64 [3, 4]            retrieve_samples_by_idx at positions 0, 33, 36: the k-step views' tags
    prio float32 [n]                                the priority vector, n = current_size
    rank int64 [n]                                  the `rank` of get_random_sample (1 + n - rankdata(.., 'ordinal'))
    alpha, beta, is_weights float64 [n]             the returned is_weights put back in position order through `filter`
    update_index int64 [5], update_prio float32 [5], prio_after float32 [37]      prios before / after update_prios
tests/test_prio_replay.py drives tetris_replay_add_dev and the other three calls against it.
Run:  python tests/golden/make_replay_golden.py        (needs /root/reference and scipy)
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/agents/agent_utils"
ADDS = (11, 17, 9, 12, 30, 5)
MAX_SIZE, K_STEP = 40, 3


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def import_replay():
    agents = types.ModuleType("agents")
    agents.__path__ = []
    utils = types.ModuleType("agents.agent_utils")
    utils.__path__ = []
    sys.modules["agents"], sys.modules["agents.agent_utils"] = agents, utils
    agents.agent_utils = utils
    utils.k_step_view = _load("agents.agent_utils.fcns", os.path.join(REF, "fcns.py")).k_step_view
    return _load("agents.agent_utils.experience_replay", os.path.join(REF, "experience_replay.py"))


def main():
    mod = import_replay()
    rep = mod.experience_replay(max_size=MAX_SIZE, k_step=K_STEP, state_size=([(None, 1)], [(None, 1)]), action_size=[[3]])
    out = {"max_size": MAX_SIZE, "k_step": K_STEP, "adds": np.array(ADDS), "slice_start": [], "slice_stop": [], "cursor": []}
    tag = 1
    for n in ADDS:
        t = np.arange(tag, tag + n).reshape(-1, 1)
        tag += n
        data = (([t], [t]), [np.repeat(t, 3, 1) % 7], (t % 3 - 1).astype(np.float32), (t % 5 == 0))
        rep.add_samples(data, 2 * np.ones((n, 1)), retrieve_samples=False)
        # the slice add_indices handed out is [current_idx - n, current_idx) (experience_replay.py:138)
        out["slice_start"].append(rep.current_idx - n)
        out["slice_stop"].append(rep.current_idx)
        out["cursor"].append((rep.current_idx, rep.current_size))
    out["ring"] = rep._visual_states[0].ravel().astype(np.int64)
    out["done"], out["reward"], out["action"] = rep._dones.ravel(), rep._rewards.ravel(), rep._actions[0]
    out["view_at"] = np.array([0, 33, 36])
    out["view"] = np.stack([rep.retrieve_samples_by_idx([int(i)])[0][1][0].ravel() for i in out["view_at"]]).astype(np.int64)
    n = rep.current_size
    rng = np.random.default_rng(20261019)
    prio = rng.random(n).astype(np.float32)
    prio[3:9] = 2.0                               # a block of equal values: what the adds leave
    prio[20:23] = prio[11]                        # equal values apart
    prio[15], prio[27] = 0.0, -0.0
    rep.prios[:n, 0] = prio
    out["prio"] = prio.copy()
    import scipy.stats
    out["rank"] = (1 + n - scipy.stats.rankdata(rep.prios[:n].ravel(), method="ordinal")).astype(np.int64)      # experience_replay.py:48
    np.random.seed(7)
    alpha, beta = 0.7, 0.6
    _, is_weights, filt = rep.get_random_sample(n, alpha=alpha, beta=beta)
    assert sorted(filt) == list(range(n))
    w = np.zeros(n)
    for idx, at in filt.items():
        w[idx] = is_weights[at, 0]
    out["alpha"], out["beta"], out["is_weights"] = alpha, beta, w
    upd = {3: 0, 30: 1, 0: 2, 34: 3, 17: 4}
    new = np.array([[0.5], [1.5], [-0.25], [3.0], [0.0]], np.float32)
    rep.update_prios(new, upd)
    out["update_index"], out["update_prio"] = np.array(list(upd)), new[list(upd.values()), 0]
    out["prio_after"] = rep.prios.ravel().copy()
    for k in ("slice_start", "slice_stop", "cursor"):
        out[k] = np.array(out[k])
    assert out["cursor"].tolist() == [[11, 11], [28, 28], [37, 37], [12, 37], [30, 30], [35, 35]]
    np.savez_compressed(os.path.join(HERE, "replay_ring.npz"), **out)
    print({k: np.asarray(v).shape for k, v in out.items()})


if __name__ == "__main__":
    main()
