"""Cost of the trajectory windows: the library calls (tetris_traj_advantages_dev, tetris_traj_record_dev through
TorchEnv.trajectory) against the same computation composed from torch ops.

    python profiles/traj_gae.py [--out DIR] [--sizes 4096,16384,65536] [--rows 32,128]    -> DIR/traj_gae.json (default profiles/traj)

Two-player 20x10 games; 4 096, 16 384 and 65 536 of them; windows of 32 and 128 rows filled with values from 2 N(0, 1), a done
with a +-1 reward on one row in 40, a bootstrap value; gamma 0.98, gae_lambda 0.96, gve_lambda 0.95.  Paths:
  torch_adv_<rows>    the backward loop over the rows with elementwise float32 ops on [2, n] accumulators (the two lambdas side
                      by side), the reset and the cut of the bootstrap by a precomputed 1 - done mask, closed by a reversed
                      cummax: 15 launches per row and 6 per call.  Checked against the library's result (1e-5) before timing.
  adv_<rows>          Trajectory.advantages
  kernel_adv_<rows>   tetris_traj_advantages_dev alone over prepared pointers: with the 22 bytes per entry (13 read: reward, two
                      values, done; 9 written: adv, target, closed) over its time against 8 TB/s (a window of back-to-back
                      launches: launch gaps are inside)
  torch_record        seven copies into the window's row (rot, trans, piece, player, the chosen entry, the two values, done)
                      and the reward from done / dead / player with gather and where
  record              Trajectory.record
A window = HIP events around 20 calls, nothing synchronised inside; five windows per path, the paths taken in turn within every
repeat, after a warm-up of every path.  The shader clock (tetris_debug_clock_khz) is read before and after each case.  Reported
per path: the windows, their median, lowest and highest (us per call)."""
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
GAMMA, GAE_LAMBDA, GVE_LAMBDA = 0.98, 0.96, 0.95
BYTES_PER_ENTRY = 22


def case(n, rows_list):
    import torch
    ti = importlib.import_module("drl-tetris_amd.torch_interop")
    pkg = ge.package()
    P, T = 2, max(rows_list)
    b = pkg.TetrisBatch(n, P, 20, 10, seeds=orc.episode_seed(np.arange(n), 0), device=0)
    b.rollout_random(1, 20)
    te = ti.TorchEnv(b)
    tr = te.trajectory(T)
    gen = torch.Generator(device="cuda").manual_seed(0)
    f32 = dict(device="cuda", dtype=torch.float32)
    tr.value.copy_(2.0 * torch.randn(2, T, n, generator=gen, **f32))
    tr.done.copy_((torch.rand(T, n, generator=gen, device="cuda") < 1.0 / 40.0).to(torch.uint8))
    tr.reward.copy_(torch.where(torch.rand(T, n, generator=gen, device="cuda") < 0.5, -1.0, 1.0) * tr.done.float())
    boot = 2.0 * torch.randn(n, generator=gen, **f32)
    lam = torch.tensor([[GAE_LAMBDA], [GVE_LAMBDA]], **f32)
    glam = torch.tensor([[GAMMA * GAE_LAMBDA], [GAMMA * GVE_LAMBDA]], **f32)
    t_adv, t_target = torch.zeros(T, n, **f32), torch.zeros(T, n, **f32)

    def torch_adv(rows):
        nd = 1.0 - tr.done[:rows].float()
        closed = tr.done[:rows].flip(0).cummax(0).values.flip(0)
        A, W = torch.zeros(2, n, **f32), torch.zeros(2, n, **f32)
        vnext = boot
        for t in range(rows - 1, -1, -1):
            v0, v1, keep = tr.value[0, t], tr.value[1, t], nd[t]
            td = tr.reward[t] + GAMMA * vnext * keep - v0
            A = A * keep * glam + td
            W = W * keep * lam + 1.0
            est = (A + v0 - v1) / W
            t_adv[t].copy_(est[0])
            torch.add(v1, est[1], out=t_target[t])
            vnext = v0
        return t_adv[:rows], t_target[:rows], closed

    def kernel_adv(rows):
        p = te._ptr
        args = (tr._traj, rows, GAMMA, GAE_LAMBDA, GVE_LAMBDA, p(boot), p(tr.adv), p(tr.target), p(tr.closed))
        return lambda: b.traj_advantages_dev(*args)

    # one acting step, so that record has a call to record
    pt = (torch.arange(n, device="cuda") % P).to(torch.uint8)
    ae = (torch.rand(n, 4, 10, 7, generator=gen, device="cuda") + 0.01).contiguous()
    se = torch.randn(n, 7, generator=gen, **f32)
    te.step_eval(ae, se, mode="pi", player=pt, seed=1, draw=0, auto_reset=True)
    row = {"k": 0}

    def next_row():
        row["k"] = (row["k"] + 1) % T
        return row["k"]

    def torch_record():
        r = next_row()
        a = tr.action[r]
        a[:, 0].copy_(te.act_rot); a[:, 1].copy_(te.act_trans); a[:, 2].copy_(te.act_piece); a[:, 3].copy_(pt)
        tr.prob[r].copy_(te.act_chosen)
        tr.value[:, r].copy_(te.act_value)
        tr.done[r].copy_(te.done)
        p = pt.long().unsqueeze(0)
        me, you = te.dead.gather(0, p)[0] != 0, te.dead.gather(0, 1 - p)[0] != 0
        base = torch.where(me & you, -1.0, you.float() - me.float())
        torch.mul(base, te.done != 0, out=tr.reward[r])

    # equal results before anything is timed
    for rows in rows_list:
        adv, target, closed = (x.clone() for x in tr.advantages(rows, GAMMA, GAE_LAMBDA, GVE_LAMBDA, bootstrap=boot))
        ta, tt, tc = torch_adv(rows)
        assert float((adv - ta).abs().max()) < 1e-5 and float((target - tt).abs().max()) < 1e-5 and torch.equal(closed, tc), rows
    tr.record(0)
    want = [x[0].clone() for x in (tr.action, tr.prob, tr.reward, tr.done)] + [tr.value[:, 0].clone()]
    row["k"] = T - 1
    torch_record()
    assert all(torch.equal(x, y) for x, y in zip(want, [tr.action[0], tr.prob[0], tr.reward[0], tr.done[0], tr.value[:, 0]]))

    paths = {}
    for rows in rows_list:
        paths[f"torch_adv_{rows}"] = lambda rows=rows: torch_adv(rows)
        paths[f"adv_{rows}"] = lambda rows=rows: tr.advantages(rows, GAMMA, GAE_LAMBDA, GVE_LAMBDA, bootstrap=boot)
        paths[f"kernel_adv_{rows}"] = kernel_adv(rows)
    paths["torch_record"] = torch_record
    paths["record"] = lambda: tr.record(next_row())
    out = {"clock_mhz": [b.clock_mhz()], "us_per_call": {}}
    for fn in paths.values():
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    windows = {name: [] for name in paths}
    for _ in range(WINDOWS):
        for name, fn in paths.items():
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
    out["kernel_bandwidth"] = {}
    for rows in rows_list:
        nbytes, t = BYTES_PER_ENTRY * n * rows, us[f"kernel_adv_{rows}"]["median"]
        out["kernel_bandwidth"][f"kernel_adv_{rows}"] = {"bytes": nbytes, "us": t, "TB_per_s": round(nbytes / t / 1e6, 3),
                                                         "share_of_8_TB_per_s": round(nbytes / t / 1e6 / (PEAK / 1e12), 4),
                                                         "us_per_row": round(t / rows, 4)}

    def versus(new, old):
        a, o = us[new], us[old]
        return {"new": new, "old": old, "faster_in_every_window": all(x < y for x, y in zip(a["windows"], o["windows"])),
                "spreads_do_not_overlap": a["max"] < o["min"], "old_over_new": round(o["median"] / a["median"], 2)}

    out["acceptance"] = [versus(f"adv_{rows}", f"torch_adv_{rows}") for rows in rows_list] + [versus("record", "torch_record")]
    out["errors"] = b.take_errors()
    b.set_stream(None, external=False)
    b.close()
    return out


def main():
    dst = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "traj")
    sizes = [int(v) for v in sys.argv[sys.argv.index("--sizes") + 1].split(",")] if "--sizes" in sys.argv else [4096, 16384, 65536]
    rows_list = [int(v) for v in sys.argv[sys.argv.index("--rows") + 1].split(",")] if "--rows" in sys.argv else [32, 128]
    out = {"note": __doc__, "calls_per_window": CALLS, "cases": {}}
    for n in sizes:
        r = case(n, rows_list)
        out["cases"][f"{n}_P2"] = r
        print(n, json.dumps({k: v["median"] for k, v in r["us_per_call"].items()}), flush=True)
        print("   ", json.dumps(r["kernel_bandwidth"]), flush=True)
        print("   ", json.dumps(r["acceptance"]), flush=True)
        os.makedirs(dst, exist_ok=True)
        with open(os.path.join(dst, "traj_gae.json"), "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
