"""Cost of one decision of a planning agent (agents/sherlock_agent/sherlock_agent.py:94-120) on the device and on the host path.

    python profiles/plan_loop.py            -> profiles/plan/plan_loop.json
    python profiles/plan_loop.py --device-only   (the device cases alone, nothing written: for a kernel-trace run)

Device (two-player 20x10 games, 4 096 and 16 384 of them, torch's stream): microseconds per call of TorchEnv.action_lists,
.simulate(finalize=False), .deltas (simulate + the field before + the torch bit unpacking), .step_lists, and of one whole
decision = action_lists + deltas + step_lists(auto_reset=True) with a choice made on the device in between; HIP events around
`reps` calls after `warmup` calls, nothing synchronised inside.  Host path (tetris_environment_vector at 256 and 4 096 games):
wall-clock seconds of get_actions + simulate_all_actions(finalize=False) + perform_action of one list per game, the loop the
device path replaces."""
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as ge  # noqa: E402
from oracle import oracle as orc  # noqa: E402


def device_case(n, warmup=5, reps=30):
    import torch
    ti = importlib.import_module("drl-tetris_amd.torch_interop")
    pkg = ge.package()
    b = pkg.TetrisBatch(n, 2, 20, 10, seeds=orc.episode_seed(np.arange(n), 0), device=0)
    b.rollout_random(1, 20)                      # boards with some stack on them
    te = ti.TorchEnv(b)
    w = torch.rand(n, 20, 10, 1, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    players = [torch.full((n,), p, dtype=torch.uint8, device="cuda") for p in (0, 1)]
    zero = torch.zeros(n, dtype=torch.int32, device="cuda")

    def decide(it):
        pt = players[it % 2]
        count, _, _ = te.action_lists(player=pt)
        d, _ = te.deltas(player=pt)
        score = (d * w).sum(dim=(1, 2)).masked_fill(torch.arange(d.shape[3], device="cuda")[None, :] >= count[:, None].long(), -1.0)
        te.step_lists(score.argmax(dim=1).to(torch.int32), player=pt, auto_reset=True)

    calls = {
        "action_lists": lambda it: te.action_lists(player=players[it % 2]),
        "simulate": lambda it: te.simulate(player=players[it % 2], finalize=False),
        "simulate_finalize": lambda it: te.simulate(player=players[it % 2], finalize=True),
        "deltas": lambda it: te.deltas(player=players[it % 2]),
        "step_lists": lambda it: te.step_lists(zero, player=players[it % 2], auto_reset=True),
        "decision": decide,
    }
    out = {}
    te.action_lists(player=players[0])
    for name, fn in calls.items():
        for it in range(warmup):
            fn(it)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for it in range(reps):
            fn(it)
        e1.record()
        e1.synchronize()
        out[name] = round(e0.elapsed_time(e1) * 1000.0 / reps, 2)
    counts = te.action_lists(player=players[0])[0]
    torch.cuda.synchronize()
    out["lists_per_game_mean"] = round(float(counts.float().mean()), 2)
    out["errors"] = b.take_errors()
    b.set_stream(None, external=False)
    b.close()
    return out


def host_case(n, reps=2):
    env_mod = importlib.import_module("drl-tetris_amd.environment")
    env = env_mod.tetris_environment_vector(n, None, settings={"n_players": 2, "game_size": [20, 10], "seed_source": lambda: 1})
    env.backend.rollout_random(1, 20)
    rng = np.random.default_rng(0)
    times = []
    for it in range(reps + 1):
        p = [it % 2] * n
        t0 = time.perf_counter()
        lists = env.get_actions(player=p)
        sims = env.simulate_all_actions(player=p, finalize=False)
        for s in sims:                           # what the agent reads: every afterstate's field
            for st in s:
                st[it % 2]["field"]
        acts = [al[int(rng.integers(len(al)))] for al in lists]
        _, dones = env.perform_action(acts, player=p)
        env.reset(env=[i for i, d in enumerate(dones) if d])
        times.append(time.perf_counter() - t0)
    return {"decision_s": round(float(np.median(times[1:])), 4), "reps": reps}


def main():
    out = {"device_us_per_call": {}, "host_path_s_per_decision": {}, "note": __doc__}
    for n in (4096, 16384):
        out["device_us_per_call"][str(n)] = device_case(n)
        print(n, out["device_us_per_call"][str(n)], flush=True)
    if "--device-only" in sys.argv:
        return
    for n in (256, 4096):
        out["host_path_s_per_decision"][str(n)] = host_case(n)
        print(n, out["host_path_s_per_decision"][str(n)], flush=True)
    dst = os.path.join(ROOT, "profiles", "plan")
    os.makedirs(dst, exist_ok=True)
    with open(os.path.join(dst, "plan_loop.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
