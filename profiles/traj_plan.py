"""Cost of a planning agent's trajectory window: the library calls (tetris_traj_record_plan_dev, tetris_traj_plan_batch_dev through
TorchEnv.trajectory(states=True, plan=True)) against what the library offered before them — the float planes of the choosing
call kept by hand in [T, n, H, 10] tensors.

    python profiles/traj_plan.py [--out DIR] [--sizes 4096,16384]    -> DIR/traj_plan.json (default profiles/traj)

Two-player 20x10 games after 20 random steps; 4 096 and 16 384 of them; 64 lists per game; a window of 128 rows, every row filled
by action_lists, observe, step_lists_eval (pi, auto-reset, float planes) and both ways of recording.  Paths:
  torch_record          two copy_ of the choosing call's delta / sums into the [T, n, H, 10] float windows, the copies of choice,
                        piece, player, pi(a), values and done into window tensors, and the reward expression on done / dead
  record_plan           Trajectory.record_plan(row)
  step_planes_torch     step_lists_eval(planes=True) + torch_record: the actor-side cost of a step before
  step_lean_record      step_lists_eval(planes=False) + record_plan: the actor-side cost of a step now
  torch_batch_plan_<M>  index_select on the two float windows and flip of the mirrored half's columns; M = 4 096 and 65 536, half
                        of the entries mirrored, a random permutation
  batch_plan_<M>        Trajectory.batch_plan(index); with the bytes it moves (read: 4 index + 448 record; written: 2 x 800) over
                        its time against 8 TB/s
Every torch composition is checked for equal bytes against the library's result before anything is timed.  A window = HIP events
around 20 calls, nothing synchronised inside; five windows per path, the paths taken in turn within every repeat, after a warm-up
of every path.  The shader clock (tetris_debug_clock_khz) is read before and after each case.  Reported per path: the windows,
their median, lowest and highest (us per call); per case the window's resident size in both forms (448 B against 1 600 B per
entry)."""
import importlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as ge  # noqa: E402
from oracle import oracle as orc  # noqa: E402

CALLS, WINDOWS, WARMUP = 20, 5, 3
PEAK = 8.0e12
T, H, P, L = 128, 20, 2, 64
BATCH_M = (4096, 65536)
BATCH_BYTES = (4 + 448) + 2 * H * 10 * 4


def case(n):
    import torch
    ti = importlib.import_module("drl-tetris_amd.torch_interop")
    pkg = ge.package()
    b = pkg.TetrisBatch(n, P, H, 10, seeds=orc.episode_seed(np.arange(n), 0), device=0)
    b.rollout_random(1, 20)
    te = ti.TorchEnv(b)
    tr = te.trajectory(T, states=True, plan=True)
    gen = torch.Generator(device="cuda").manual_seed(0)
    u8, f32 = dict(device="cuda", dtype=torch.uint8), dict(device="cuda", dtype=torch.float32)
    w_delta, w_sums = torch.zeros(T, n, H, 10, **f32), torch.zeros(T, n, H, 10, **f32)
    w_action, w_prob, w_value = torch.zeros(T, n, 4, **u8), torch.zeros(T, n, **f32), torch.zeros(2, T, n, **f32)
    w_reward, w_done = torch.zeros(T, n, **f32), torch.zeros(T, n, **u8)
    player = (torch.arange(n, device="cuda") % P).to(torch.uint8)
    pl = player.long()[None]
    zero = torch.zeros(n, **u8)
    phi = torch.rand(n, H, 10, 7, generator=gen, device="cuda") + 0.1
    se = torch.randn(n, 7, generator=gen, device="cuda")
    last = {}

    def step(row, planes):
        out = te.step_lists_eval(phi, se, mode="pi", player=player, seed=1, draw=row, auto_reset=True, planes=planes)
        if planes:
            last["out"] = out

    def torch_record(row):
        done, _, dead, choice, piece, prob, value, _, delta, sums = last["out"]
        w_delta[row].copy_(delta); w_sums[row].copy_(sums)
        w_action[row].copy_(torch.stack([choice.to(torch.uint8), zero, piece, player], dim=1))
        w_prob[row].copy_(prob); w_value[:, row].copy_(value); w_done[row].copy_(done)
        me, you = dead.gather(0, pl)[0] != 0, dead.gather(0, 1 - pl)[0] != 0
        w_reward[row].copy_(torch.where(done != 0, torch.where(me & you, -1.0, you.float() - me.float()), 0.0))

    for row in range(T):
        te.action_lists(player=player, max_lists=L)
        tr.observe(row, player)
        step(row, True)
        torch_record(row)
        tr.record_plan(row)
    # equal results before anything is timed
    torch.cuda.synchronize()
    for name, mine in (("action", w_action), ("prob", w_prob), ("value", w_value), ("reward", w_reward), ("done", w_done)):
        assert torch.equal(getattr(tr, name).view(torch.uint8), mine.view(torch.uint8)), name
    assert bool((w_done != 0).any()) and bool((w_delta != 0).any())
    mirror_bit = -(1 << 31)

    def torch_batch_plan(index):
        at = (index & 0x7FFFFFFF).long()
        mir = (index < 0).view(-1, 1, 1)
        out = []
        for wdw in (w_delta, w_sums):
            v = wdw.view(T * n, H, 10).index_select(0, at)
            out.append(torch.where(mir, v.flip(2), v))
        return out

    indices = {}
    for M in BATCH_M:
        at = torch.randint(0, T * n, (M,), generator=gen, device="cuda", dtype=torch.int32)
        indices[M] = torch.where(torch.rand(M, generator=gen, device="cuda") < 0.5, at | mirror_bit, at).contiguous()
        got, want = tr.batch_plan(indices[M]), torch_batch_plan(indices[M])
        for name, g, w in zip(got._fields, got, want):
            assert torch.equal(g[..., 0].view(torch.int32), w.contiguous().view(torch.int32)), (M, name)
        share = float((indices[M] < 0).float().mean())
        assert 0.4 < share < 0.6, share
    row = {"k": 0}

    def next_row():
        row["k"] = (row["k"] + 1) % T
        return row["k"]

    def step_planes_torch():
        r = next_row()
        step(r, True)
        torch_record(r)

    def step_lean_record():
        r = next_row()
        step(r, False)
        tr.record_plan(r)

    paths = {"torch_record": lambda: torch_record(next_row()), "record_plan": lambda: tr.record_plan(next_row()),
             "step_planes_torch": step_planes_torch, "step_lean_record": step_lean_record}
    for M in BATCH_M:
        paths[f"torch_batch_plan_{M}"] = lambda M=M: torch_batch_plan(indices[M])
        paths[f"batch_plan_{M}"] = lambda M=M: tr.batch_plan(indices[M])
    out = {"clock_mhz": [b.clock_mhz()], "us_per_call": {}}
    out["window_resident_bytes"] = {"rows": T, "plan_records": tr.plan_rec.numel() * 4, "float_planes": (w_delta.numel() + w_sums.numel()) * 4,
                                    "per_entry": {"plan_record": 448, "float_planes": 2 * H * 10 * 4}}
    for fn in paths.values():
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    windows = {name: [] for name in paths}
    for _ in range(WINDOWS):
        for name, fn in paths.items():
            te.action_lists(player=player, max_lists=L)                 # (the lists of the boards as they are now; not timed)
            tr.observe(row["k"], player)
            step(row["k"], True)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(CALLS):
                fn()
            e1.record()
            e1.synchronize()
            windows[name].append(round(e0.elapsed_time(e1) * 1000.0 / CALLS, 2))
    us = out["us_per_call"]
    for name, ws in windows.items():
        us[name] = {"windows": ws, "median": statistics.median(ws), "min": min(ws), "max": max(ws)}
    out["clock_mhz"].append(b.clock_mhz())
    out["batch_bandwidth"] = {}
    for M in BATCH_M:
        nbytes, t = BATCH_BYTES * M, us[f"batch_plan_{M}"]["median"]
        out["batch_bandwidth"][f"batch_plan_{M}"] = {"bytes": nbytes, "us": t, "TB_per_s": round(nbytes / t / 1e6, 3),
                                                     "share_of_8_TB_per_s": round(nbytes / t / 1e6 / (PEAK / 1e12), 4)}

    def versus(new, old):
        a, o = us[new], us[old]
        return {"new": new, "old": old, "faster_in_every_window": all(x < y for x, y in zip(a["windows"], o["windows"])),
                "spreads_do_not_overlap": a["max"] < o["min"], "old_over_new": round(o["median"] / a["median"], 2)}

    out["comparison"] = ([versus("record_plan", "torch_record"), versus("step_lean_record", "step_planes_torch")]
                         + [versus(f"batch_plan_{M}", f"torch_batch_plan_{M}") for M in BATCH_M])
    out["errors"] = b.take_errors()
    b.set_stream(None, external=False)
    b.close()
    return out


def main():
    dst = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "traj")
    sizes = [int(v) for v in sys.argv[sys.argv.index("--sizes") + 1].split(",")] if "--sizes" in sys.argv else [4096, 16384]
    out = {"note": __doc__, "calls_per_window": CALLS, "cases": {}}
    for n in sizes:
        r = case(n)
        out["cases"][f"{n}_P2"] = r
        print(n, json.dumps({k: v["median"] for k, v in r["us_per_call"].items()}), flush=True)
        print("   ", json.dumps(r["batch_bandwidth"]), flush=True)
        print("   ", json.dumps(r["comparison"]), flush=True)
        os.makedirs(dst, exist_ok=True)
        with open(os.path.join(dst, "traj_plan.json"), "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
