"""Cost of the device-side heuristic policy (include/tetris_hip.h: tetris_rt_features_dev .. tetris_rollout_policy) and of the
same decision composed from what the library offered before it.

    python profiles/policy_loop.py                 -> profiles/policy/policy_loop.json
    python profiles/policy_loop.py --device-only   (a few calls of everything, nothing written: for a kernel-trace run)
    python profiles/policy_loop.py --merge-trace DIR   (adds the per-kernel rows of rocprofv3 --kernel-trace --stats output
                                                        found under DIR to the JSON)
    python profiles/policy_loop.py --rehearse      (no GPU: checks the composition's torch features against numpy)

Per (games, players) in 4 096 / 65 536 x 1 / 2, 20x10 boards after 40 steps of the policy itself, torch's stream, HIP events
around `calls` calls after a warm-up, nothing synchronised inside; `repeats` windows per path, the paths taken in turn inside
every repeat so that all of them see the same machine state; median, min and max over the windows:
  rt_features, policy_rt, step_policy (auto-reset)      TorchEnv calls
  composed      the yardstick: the 40 key lists [8]*r + [2] + [3]*t + [7] written once into [N][40][16] buffers,
                tetris_simulate_lists_dev, the eight features from d_cols in torch (bit unpacking, as TorchEnv.deltas does),
                argmax, tetris_step_rt_dev_ex — the same decision and step without the new kernels
  rollout_policy   per env-step of one batch step, steps_per_launch 1 (spread mapping: 40 N lanes evaluate, N lanes choose and
                step) and 8 (lane mapping: every lane evaluates its own 40 candidates), from the call's own HIP-event time;
                env-steps/s and lines per step from its counters.
The shader clock (tetris_debug_clock_khz) is noted before and after every case."""
import glob
import importlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "policy", "policy_loop.json")
WEIGHTS = (34, -79, 0, -10, 0, -32, -93, -34)
K = 16                                       # keys per list: 3 rotations + [2] + 9 translations + [7] = 14


def torch_features(cols, H):
    """cols int32 [40, 10, N] (bit y = row y) -> int32 [40, 8, N]: the feature table of include/tetris_hip.h in torch"""
    import torch
    L, W, N = cols.shape
    rows = torch.arange(H, dtype=torch.int32, device=cols.device)
    f = torch.bitwise_and(torch.bitwise_right_shift(cols.unsqueeze(-1), rows), 1).bool()        # [L, W, N, H]
    full = f.all(dim=1)                                                                          # [L, N, H]
    lines = full.sum(dim=-1)
    # full rows removed, the rows above moved down: a stable sort of the rows that puts the full ones on top, then cleared
    order = torch.argsort(full.logical_not().to(torch.uint8), dim=-1, stable=True)               # [L, N, H]
    g = torch.gather(f, 3, order.unsqueeze(1).expand(L, W, N, H))
    g = g & (rows.view(1, 1, 1, H) >= lines.view(L, 1, N, 1))
    any_ = g.any(dim=-1)
    top = g.to(torch.uint8).argmax(dim=-1)
    h = torch.where(any_, H - top, torch.zeros_like(top))                                        # [L, W, N]
    below = torch.cumsum(g.to(torch.int32), dim=-1) > 0
    holes = (below & ~g).sum(dim=(1, 3))
    bump = (h[:, 1:] - h[:, :-1]).abs().sum(dim=1)
    agg = h.sum(dim=1)
    mx = h.max(dim=1).values
    wall = torch.ones((L, 1, N, H), dtype=torch.bool, device=cols.device)
    padded = torch.cat([wall, g, wall], dim=1)
    rowtr = (padded[:, 1:] != padded[:, :-1]).sum(dim=(1, 3))
    floor = torch.ones((L, W, N, 1), dtype=torch.bool, device=cols.device)
    padv = torch.cat([g, floor], dim=3)
    coltr = (padv[..., 1:] != padv[..., :-1]).sum(dim=(1, 3))
    edge = torch.full((L, 1, N), H, dtype=h.dtype, device=cols.device)
    hp = torch.cat([edge, h, edge], dim=1)
    d = (torch.minimum(hp[:, :-2], hp[:, 2:]) - h).clamp(min=0)
    wells = (d * (d + 1) // 2).sum(dim=1)
    return torch.stack([lines, holes, bump, agg, mx, rowtr, coltr, wells], dim=1).to(torch.int32)


def rehearse():
    """host side of the composition against numpy, no GPU"""
    import torch
    rng = np.random.default_rng(0)
    H, N = 20, 6
    f = rng.random((40, N, H, 10)) < 0.55
    f[:, :, 15:17, :] |= rng.random((40, N, 2, 10)) < 0.9                  # some full rows
    cols = (f.transpose(0, 3, 1, 2).astype(np.int64) << np.arange(H)).sum(axis=-1).astype(np.int32)      # [40, 10, N]
    from tests.policy_model import features
    want = features(f.reshape(40 * N, H, 10)).reshape(40, N, 8).transpose(0, 2, 1)
    got = torch_features(torch.from_numpy(cols), H).numpy()
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert (want[:, 0] > 0).any()
    print("rehearsal ok: torch features equal numpy on", 40 * N, "random fields")


def timed(fn, calls, torch):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for it in range(calls):
        fn(it)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def case(n, P, repeats, short=False):
    import torch
    import __graft_entry__ as ge
    from oracle import oracle as orc
    ti = importlib.import_module("drl-tetris_amd.torch_interop")
    b = ge.package().TetrisBatch(n, P, 20, 10, seeds=orc.episode_seed(np.arange(n), 0), device=0)
    w = torch.tensor(WEIGHTS, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    b.rollout_policy(w.data_ptr(), 40, 1)                                  # boards that look like play
    clock0 = b.clock_mhz()
    te = ti.TorchEnv(b)
    players = [torch.full((n,), p, dtype=torch.uint8, device="cuda") for p in range(P)]
    # the composition's buffers: the 40 key lists of every game, written once
    keys = np.zeros((40, K), np.uint8)
    lens = np.zeros(40, np.uint8)
    for c in range(40):
        k = [8] * (c // 10) + [2] + [3] * (c % 10) + [7]
        keys[c, :len(k)] = k
        lens[c] = len(k)
    d_keys = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(keys, (n, 40, K)))).cuda()
    d_lens = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(lens, (n, 40)))).cuda()
    d_count = torch.full((n,), 40, dtype=torch.int32, device="cuda")
    d_cols = torch.zeros(40, P, 10, n, dtype=torch.int32, device="cuda")
    wl = w.to(torch.int32).view(1, 8, 1)
    C = te._ptr

    def composed_features(it):
        p = it % P
        b.simulate_lists_dev(C(d_count), C(d_lens), C(d_keys), C(d_cols), max_lists=40, max_keys=K, player=C(players[p]))
        return torch_features(d_cols[:, p], 20)

    def composed(it):
        best = (composed_features(it) * wl).sum(dim=1).argmax(dim=0)                 # [N]
        te.step_rt((best // 10).to(torch.uint8), (best % 10).to(torch.uint8), player=players[it % P], auto_reset=True)

    same = bool(torch.equal(composed_features(0), te.rt_features(players[0]).to(torch.int32)))
    paths = {
        "rt_features": (lambda it: te.rt_features(players[it % P]), 20),
        "policy_rt": (lambda it: te.policy_rt(w, players[it % P]), 20),
        "step_policy": (lambda it: te.step_policy(w, players[it % P], auto_reset=True), 20),
        "composed": (composed, 3),
    }
    if short:
        for fn, _ in paths.values():
            for it in range(2):
                fn(it)
        torch.cuda.synchronize()
        b.set_stream(0, external=False)
        b.rollout_policy(w.data_ptr(), 4, 1)
        b.rollout_policy(w.data_ptr(), 1, 8, first_step=4)
        b.close()
        return None
    windows = {name: [] for name in paths}
    for name, (fn, calls) in paths.items():                                         # warm-up of every shape
        timed(fn, 2, torch)
    for rep in range(repeats):
        for name, (fn, calls) in paths.items():
            windows[name].append(timed(fn, calls, torch))
    out = {"composed_features_equal_rt_features": same}
    for name, v in windows.items():
        out[name] = {"us_per_call_median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2), "windows": len(v)}
    out["step_policy_speedup_over_composed"] = round(out["composed"]["us_per_call_median"] / out["step_policy"]["us_per_call_median"], 2)
    torch.cuda.synchronize()
    b.set_stream(0, external=False)                                                 # the rollout runs on the batch's own stream
    step = 0
    for spl, launches in ((1, 256), (8, 32)):
        b.rollout_policy(w.data_ptr(), 16, spl, first_step=step)                    # warm-up
        step += 16 * spl
        us, rates, lines = [], [], []
        for rep in range(repeats):
            counters, ms = b.rollout_policy(w.data_ptr(), launches, spl, first_step=step)
            step += launches * spl
            us.append(ms * 1e3 / (launches * spl))
            rates.append(float(counters[0]) / (ms * 1e-3))
            lines.append(float(counters[2]) / float(counters[0]))
        out[f"rollout_policy_spl{spl}"] = {"us_per_step_median": round(statistics.median(us), 2), "min": round(min(us), 2), "max": round(max(us), 2),
                                           "env_steps_per_s_median": round(statistics.median(rates)), "lines_per_env_step": round(statistics.median(lines), 4),
                                           "windows": len(us)}
    out["errors"] = b.take_errors()
    out["shader_clock_mhz"] = [round(clock0), round(b.clock_mhz())]
    b.close()
    return out


def merge_trace(d):
    """per-kernel rows (name, calls, total / average ns) of rocprofv3 --kernel-trace --stats -> the JSON"""
    import csv
    rows = []
    for fn in sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)):
        for r in csv.DictReader(open(fn)):
            rows.append({"kernel": r.get("Name", "")[:120], "calls": int(r.get("Calls", 0)), "total_ns": int(float(r.get("TotalDurationNs", 0))),
                         "average_ns": round(float(r.get("AverageNs", 0)), 1), "percent": round(float(r.get("Percentage", 0)), 2)})
    res = json.load(open(OUT))
    res["kernel_trace_stats"] = {"command": "rocprofv3 --kernel-trace --stats -- python profiles/policy_loop.py --device-only", "rows": rows}
    json.dump(res, open(OUT, "w"), indent=1)
    print(f"{len(rows)} kernel rows merged into {OUT}")


if __name__ == "__main__":
    if "--rehearse" in sys.argv:
        rehearse()
        sys.exit(0)
    if "--merge-trace" in sys.argv:
        merge_trace(sys.argv[sys.argv.index("--merge-trace") + 1])
        sys.exit(0)
    short = "--device-only" in sys.argv
    res = {"note": __doc__, "weights": list(WEIGHTS), "cases": {}}
    for n in ((65536,) if short else (4096, 65536)):           # (the kernel-trace run: the large size only)
        for P in (1, 2):
            r = case(n, P, repeats=5, short=short)
            if r is not None:
                res["cases"][f"{n}x{P}"] = r
                print(n, P, json.dumps(r), flush=True)
    if not short:
        import __graft_entry__ as ge
        res["device"] = ge.package().capi.device_name(0)
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        json.dump(res, open(OUT, "w"), indent=1)
        print("wrote", OUT)
