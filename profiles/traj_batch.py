"""Cost of a trajectory window's states and sample sets: the library calls (tetris_traj_observe_dev, tetris_traj_select_dev,
tetris_traj_batch_dev through TorchEnv.trajectory(states=True)) against the same results composed from torch ops on the calls the
library had before them.

    python profiles/traj_batch.py [--out DIR] [--sizes 4096,16384,65536]    -> DIR/traj_batch.json (default profiles/traj)

Two-player 20x10 games after 20 random steps; 4 096, 16 384 and 65 536 of them; a window of 128 rows, every row observed after
one more random step (auto-reset); `closed` as advantages leaves it with a done on one row in 40.  Paths:
  torch_observe       three copies of the TorchEnv's visual / vector / piece (as step_eval_observe leaves them) into [T, ...] byte
                      tensors
  observe             Trajectory.observe(row)
  torch_select_<rows> nonzero on closed[:rows] + cat of the list and the list with bit 31 set
  select_<rows>       Trajectory.select(rows, augment=True)
  torch_batch_<M>     index_select on the byte tensors, flip of the mirrored half's columns, the piece / next / action remaps and
                      the seven scalar gathers; M = 4 096 and 65 536, half of the entries mirrored, a random permutation
  batch_<M>           Trajectory.batch(index); with the bytes it moves (read: 4 index + 96 record + 4 action + 12 floats + 1 done;
                      written: 426 planes + 3 + 16 + 2) over its time against 8 TB/s
Every torch composition is checked for equal bytes against the library's result before anything is timed.  A window = HIP events
around 20 calls, nothing synchronised inside; five windows per path, the paths taken in turn within every repeat, after a warm-up
of every path.  The shader clock (tetris_debug_clock_khz) is read before and after each case.  Reported per path: the windows,
their median, lowest and highest (us per call); per case the window's resident size in both forms."""
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
T, H, P = 128, 20, 2
SELECT_ROWS, BATCH_M = (32, 128), (4096, 65536)
BATCH_BYTES = (4 + 96 + 4 + 12 + 1) + (426 + 3 + 16 + 2)


def case(n):
    import torch
    ti = importlib.import_module("drl-tetris_amd.torch_interop")
    pkg = ge.package()
    b = pkg.TetrisBatch(n, P, H, 10, seeds=orc.episode_seed(np.arange(n), 0), device=0)
    b.rollout_random(1, 20)
    te = ti.TorchEnv(b)
    tr = te.trajectory(T, states=True)
    gen = torch.Generator(device="cuda").manual_seed(0)
    u8 = dict(device="cuda", dtype=torch.uint8)
    w_visual, w_vector, w_piece = torch.zeros(T, P, n, H, 10, **u8), torch.zeros(T, P, n, 12, **u8), torch.zeros(T, P, n, **u8)
    player = (torch.arange(n, device="cuda") % P).to(torch.uint8)

    def torch_observe(row):           # (the observation itself is there already: step_eval_observe wrote it)
        w_visual[row].copy_(te.visual); w_vector[row].copy_(te.vector); w_piece[row].copy_(te.piece)

    for row in range(T):
        rot = torch.randint(0, 4, (n,), generator=gen, device="cuda").to(torch.uint8)
        trans = torch.randint(0, 10, (n,), generator=gen, device="cuda").to(torch.uint8)
        te.step_rt(rot, trans, player, auto_reset=True)
        te.observe(player)
        torch_observe(row)
        tr.observe(row, player)
    tr.action.copy_(torch.stack([torch.randint(0, hi, (T, n), generator=gen, device="cuda") for hi in (4, 10, 7, 2)], dim=2).to(torch.uint8))
    for x in (tr.prob, tr.reward, tr.adv, tr.target):
        x.copy_(torch.randn(T, n, generator=gen, device="cuda"))
    tr.done.copy_((torch.rand(T, n, generator=gen, device="cuda") < 1.0 / 40.0).to(torch.uint8))
    tr.closed.copy_(tr.done.flip(0).cummax(0).values.flip(0))
    tr._rows = T
    swap = torch.tensor([1, 0, 3, 2, 4, 5, 6, 7], **u8)
    mirror_bit = -(1 << 31)

    def torch_select(rows):
        k = tr.closed[:rows].reshape(-1).nonzero().reshape(-1).to(torch.int32)
        return torch.cat([k, k | mirror_bit])

    def torch_batch(index):
        at = (index & 0x7FFFFFFF).long()
        mir = index < 0
        t, i = at // n, at % n
        flat = t * (P * n) + i                                      # slot 0 of entry (t, i) in the [T * P * n, ...] views
        out = []
        vis_v, vec_v, pc_v = w_visual.view(T * P * n, H, 10), w_vector.view(T * P * n, 12), w_piece.view(T * P * n)
        vis, vec, pc = [], [], []
        for sl in range(P):
            v = vis_v.index_select(0, flat + sl * n)
            vis.append(torch.where(mir.view(-1, 1, 1), v.flip(2), v))
            x = vec_v.index_select(0, flat + sl * n)
            x[:, 5:] = torch.where(mir.view(-1, 1), 1 - x[:, 5:], x[:, 5:])
            vec.append(x)
            q = pc_v.index_select(0, flat + sl * n)
            pc.append(torch.where(mir, swap[q.long()], q))
        a = tr.action.view(T * n, 4).index_select(0, at)
        act = torch.stack([a[:, 0], torch.where(mir, 9 - a[:, 1], a[:, 1]), torch.where(mir, swap[a[:, 2].long()], a[:, 2])], dim=1)
        out = [torch.stack(vis), torch.stack(vec), torch.stack(pc), act]
        out += [x.view(-1).index_select(0, at) for x in (tr.prob, tr.adv, tr.target, tr.reward, tr.done)]
        return out

    # equal results before anything is timed
    lists = {}
    for rows in SELECT_ROWS:
        index, count = tr.select(rows, augment=True)
        want = torch_select(rows)
        assert int(count.item()) == want.numel() and torch.equal(index[:want.numel()], want), rows
        lists[rows] = want
    indices = {}
    for M in BATCH_M:
        pool = lists[T]
        indices[M] = pool[torch.randint(0, pool.numel(), (M,), generator=gen, device="cuda")].contiguous()
        got, want = tr.batch(indices[M]), torch_batch(indices[M])
        for name, g, w in zip(got._fields, got, want):
            assert torch.equal(g.view(torch.uint8), w.contiguous().view(torch.uint8)), (M, name)
        assert bool(got.valid.all())
        share = float((indices[M] < 0).float().mean())
        assert 0.4 < share < 0.6, share
    row = {"k": 0}

    def next_row():
        row["k"] = (row["k"] + 1) % T
        return row["k"]

    paths = {"torch_observe": lambda: torch_observe(next_row()), "observe": lambda: tr.observe(next_row(), player)}
    for rows in SELECT_ROWS:
        paths[f"torch_select_{rows}"] = lambda rows=rows: torch_select(rows)
        paths[f"select_{rows}"] = lambda rows=rows: tr.select(rows, augment=True)
    for M in BATCH_M:
        paths[f"torch_batch_{M}"] = lambda M=M: torch_batch(indices[M])
        paths[f"batch_{M}"] = lambda M=M: tr.batch(indices[M])
    out = {"clock_mhz": [b.clock_mhz()], "us_per_call": {}}
    out["window_resident_bytes"] = {"rows": T, "packed_records": tr.obs.numel() * 4, "byte_planes": w_visual.numel() + w_vector.numel() + w_piece.numel()}
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
    out["batch_bandwidth"] = {}
    for M in BATCH_M:
        nbytes, t = BATCH_BYTES * M, us[f"batch_{M}"]["median"]
        out["batch_bandwidth"][f"batch_{M}"] = {"bytes": nbytes, "us": t, "TB_per_s": round(nbytes / t / 1e6, 3),
                                                "share_of_8_TB_per_s": round(nbytes / t / 1e6 / (PEAK / 1e12), 4)}

    def versus(new, old):
        a, o = us[new], us[old]
        return {"new": new, "old": old, "faster_in_every_window": all(x < y for x, y in zip(a["windows"], o["windows"])),
                "spreads_do_not_overlap": a["max"] < o["min"], "old_over_new": round(o["median"] / a["median"], 2)}

    out["comparison"] = ([versus("observe", "torch_observe")] + [versus(f"select_{rows}", f"torch_select_{rows}") for rows in SELECT_ROWS]
                         + [versus(f"batch_{M}", f"torch_batch_{M}") for M in BATCH_M])
    out["errors"] = b.take_errors()
    b.set_stream(None, external=False)
    b.close()
    return out


def main():
    dst = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "traj")
    sizes = [int(v) for v in sys.argv[sys.argv.index("--sizes") + 1].split(",")] if "--sizes" in sys.argv else [4096, 16384, 65536]
    out = {"note": __doc__, "calls_per_window": CALLS, "cases": {}}
    for n in sizes:
        r = case(n)
        out["cases"][f"{n}_P2"] = r
        print(n, json.dumps({k: v["median"] for k, v in r["us_per_call"].items()}), flush=True)
        print("   ", json.dumps(r["batch_bandwidth"]), flush=True)
        print("   ", json.dumps(r["comparison"]), flush=True)
        os.makedirs(dst, exist_ok=True)
        with open(os.path.join(dst, "traj_batch.json"), "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
