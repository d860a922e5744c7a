"""Cost of the deltas of a planning agent: the one-kernel path (tetris_plan_deltas_dev) against the torch arithmetic it replaced.

    python profiles/plan_deltas.py [--out DIR]    -> DIR/plan_deltas.json (default profiles/plan)
    python profiles/plan_deltas.py --trace        (the new paths alone, a few calls, nothing written: for a kernel-trace run)

Two-player 20x10 games after 20 random steps, 4 096 and 16 384 of them, 64 lists, torch's stream.  Paths:
  parent             TorchEnv.simulate(finalize=False) + the packed observation + torch_interop.columns_to_deltas (what
                     TorchEnv.deltas was before the kernel; still callable)
  deltas             TorchEnv.deltas: simulate + k_plan_deltas, float32 lists-last (the default form)
  deltas_list_major, deltas_f16, deltas_f16_list_major   the other three forms
  kernel             tetris_plan_deltas_dev alone, default form (no simulate)
  simulate           TorchEnv.simulate(finalize=False) alone
  decision           action_lists + deltas + a choice made in torch + step_lists(auto_reset=True)
A window = HIP events around 20 calls, nothing synchronised inside; five windows per path, the paths taken in turn within
every repeat, after a warm-up of every path.  The shader clock (tetris_debug_clock_khz) is read before and after each size.
Reported per path: the windows, their median, lowest and highest (us per call); for the paths that are one k_plan_deltas plus
at most a simulate, the bytes the kernel writes (deltas + sums + small) over (path - simulate) against 8 TB/s."""
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

L, CALLS, WINDOWS, WARMUP = 64, 20, 5, 3
PEAK = 8.0e12


def case(n, trace=False):
    import torch
    ti = importlib.import_module("drl-tetris_amd.torch_interop")
    pkg = ge.package()
    b = pkg.TetrisBatch(n, 2, 20, 10, seeds=orc.episode_seed(np.arange(n), 0), device=0)
    b.rollout_random(1, 20)
    te = ti.TorchEnv(b)
    H = b.height
    pt = (torch.arange(n, device="cuda") % 2).to(torch.uint8)
    te.action_lists(player=pt, max_lists=L)
    w = torch.rand(n, H, 10, 1, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    old_out = torch.zeros(n, H, 10, L, dtype=torch.float32, device="cuda")
    visual, vector, piece = (torch.zeros(s, dtype=torch.uint8, device="cuda") for s in ((2, n, H, 10), (2, n, 12), (2, n)))

    def parent():
        cols = te.simulate(pt, finalize=False)[0]
        b._check(b.lib.tetris_observe_packed_dev(b._h, None, n, te._ptr(pt), te._ptr(visual), te._ptr(vector), te._ptr(piece)))
        return ti.columns_to_deltas(cols, pt, visual[0], te.list_count, H, out=old_out)

    def kernel():
        d, s = te._plan_delta_bufs[(torch.float32, False)]
        b.plan_deltas_dev(te._ptr(te.list_count), te._ptr(te.sim_cols), te._ptr(d), sums=te._ptr(s), small=te._ptr(te.plan_small),
                          max_lists=L, player=te._ptr(pt))

    def decision():
        count, _, _ = te.action_lists(player=pt, max_lists=L)
        d, _ = te.deltas(player=pt)
        score = (d * w).sum(dim=(1, 2)).masked_fill(torch.arange(L, device="cuda")[None, :] >= count[:, None].long(), -1.0)
        te.step_lists(score.argmax(dim=1).to(torch.int32), player=pt, auto_reset=True)

    paths = {
        "parent": parent,
        "deltas": lambda: te.deltas(player=pt),
        "deltas_list_major": lambda: te.deltas(player=pt, list_major=True),
        "deltas_f16": lambda: te.deltas(player=pt, dtype=torch.float16),
        "deltas_f16_list_major": lambda: te.deltas(player=pt, dtype=torch.float16, list_major=True),
        "kernel": kernel,
        "simulate": lambda: te.simulate(pt, finalize=False),
    }
    if trace:
        del paths["parent"]
        for fn in paths.values():
            for _ in range(WARMUP):
                fn()
        torch.cuda.synchronize()
        b.set_stream(None, external=False)
        b.close()
        return None
    # same numbers from both paths before anything is timed
    new_d, new_s = te.deltas(player=pt)
    want_d, want_s = parent()
    assert torch.equal(new_d, want_d) and torch.allclose(new_s, want_s, rtol=1e-6, atol=1e-6)
    clock0 = b.clock_mhz()
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
    # the whole decision last: it steps the games
    for _ in range(WARMUP):
        decision()
    torch.cuda.synchronize()
    windows["decision"] = []
    for _ in range(WINDOWS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            decision()
        e1.record()
        e1.synchronize()
        windows["decision"].append(round(e0.elapsed_time(e1) * 1000.0 / CALLS, 2))
    clock1 = b.clock_mhz()
    out = {"clock_mhz": [clock0, clock1], "us_per_call": {}}
    for name, ws in windows.items():
        out["us_per_call"][name] = {"windows": ws, "median": statistics.median(ws), "min": min(ws), "max": max(ws)}
    sim = out["us_per_call"]["simulate"]["median"]
    cells = n * H * 10
    out["kernel_bytes_over_time"] = {}
    for name, esize, minus in (("kernel", 4, 0.0), ("deltas", 4, sim), ("deltas_list_major", 4, sim), ("deltas_f16", 2, sim),
                               ("deltas_f16_list_major", 2, sim)):
        nbytes = cells * L * esize + cells * esize + n * L
        us = out["us_per_call"][name]["median"] - minus
        out["kernel_bytes_over_time"][name] = {"bytes_written": nbytes, "us": round(us, 2), "TB_per_s": round(nbytes / us / 1e6, 3),
                                               "share_of_8_TB_per_s": round(nbytes / us / 1e6 / (PEAK / 1e12), 3)}
    new, old = out["us_per_call"]["deltas"], out["us_per_call"]["parent"]
    out["acceptance"] = {"faster_in_every_window": all(a < b_ for a, b_ in zip(new["windows"], old["windows"])),
                         "spreads_do_not_overlap": new["max"] < old["min"],
                         "parent_over_new": round(old["median"] / new["median"], 2)}
    out["errors"] = b.take_errors()
    b.set_stream(None, external=False)
    b.close()
    return out


def main():
    trace = "--trace" in sys.argv
    dst = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "plan")
    out = {"note": __doc__, "lists": L, "calls_per_window": CALLS, "games": {}}
    for n in (4096, 16384):
        r = case(n, trace)
        if r is not None:
            out["games"][str(n)] = r
            print(n, json.dumps(r["us_per_call"]), json.dumps(r["acceptance"]), flush=True)
    if trace:
        return
    os.makedirs(dst, exist_ok=True)
    with open(os.path.join(dst, "plan_deltas.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
