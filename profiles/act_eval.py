"""Cost of acting on a network's (r, t, piece) evaluation: the library calls (tetris_select_eval_dev, tetris_step_eval_dev,
tetris_step_eval_observe_dev through TorchEnv) against the same decision composed from torch ops on the API the library had
before them.

    python profiles/act_eval.py [--out DIR] [--sizes 4096,16384,65536]    -> DIR/act_eval.json (default profiles/act)

20x10 games after 20 random steps; 4 096, 16 384 and 65 536 of them, one and two players, float32 and float16 evaluations,
K = 7, torch's stream.  Paths, per mode (argmax, pi, rank with theta = 1, epsilon = 0.1):
  torch_<mode>     observe()'s piece, a gather of the piece's map, argmax / multinomial / double argsort + multinomial /
                   rand + randint + argmax, the unravel to uint8 (r, t)
  select_<mode>    TorchEnv.select_eval
  kernel_<mode>    tetris_select_eval_dev alone over a prepared argument struct: with the bytes of action_eval over its time
                   against 8 TB/s (a window of back-to-back launches: launch gaps are inside)
and for pi and argmax
  torch_step_<mode>      torch_<mode> + TorchEnv.step_rt(auto_reset)
  step_<mode>            TorchEnv.step_eval
  torch_step_obs_<mode>  torch_<mode> + TorchEnv.step_rt_observe
  step_obs_<mode>        TorchEnv.step_eval_observe
A window = HIP events around 20 calls, nothing synchronised inside; five windows per path, the paths taken in turn within every
repeat, after a warm-up of every path.  (profiles/act/fused_step_and_rank_lane.json is this script's output for an earlier build
in which step_eval was ONE kernel — its step_<mode> against two_step_<mode> = select_eval + step_rt — and RANK could also be
ranked in each game's own lane — kernel_rank_lane against kernel_rank: both lost and were removed.)  The shader clock
(tetris_debug_clock_khz) is read before and after each case.  Reported per path: the windows, their median, lowest and highest
(us per call)."""
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
MODES = ("argmax", "pi", "rank", "epsilon")
EPSILON = 0.1


def case(n, P, dtype_name):
    import torch
    ti = importlib.import_module("drl-tetris_amd.torch_interop")
    pkg = ge.package()
    dtype = getattr(torch, dtype_name)
    b = pkg.TetrisBatch(n, P, 20, 10, seeds=orc.episode_seed(np.arange(n), 0), device=0)
    b.rollout_random(1, 20)
    te = ti.TorchEnv(b)
    gen = torch.Generator(device="cuda").manual_seed(0)
    pt = (torch.arange(n, device="cuda") % P).to(torch.uint8)
    ae = (torch.rand(n, 4, 10, 7, device="cuda", generator=gen) + 0.01).to(dtype).contiguous()
    table_np = pkg.capi.pareto_table(1.0)
    table = torch.from_numpy(table_np).cuda()
    state = {"draw": 0}

    def torch_choice(mode):
        piece = te.observe(pt)[2][0]
        x = ae.view(n, 40, 7).gather(2, piece.long().view(n, 1, 1).expand(n, 40, 1)).squeeze(2).float()
        if mode == "argmax":
            c = x.argmax(dim=1)
        elif mode == "pi":
            c = torch.multinomial(x.clamp_min(0.0), 1).squeeze(1)
        elif mode == "rank":
            ranks = torch.argsort(torch.argsort(-x, dim=1, stable=True), dim=1, stable=True)
            c = torch.multinomial(table[ranks], 1).squeeze(1)
        else:
            greedy = x.argmax(dim=1)
            c = torch.where(torch.rand(n, device="cuda") < EPSILON, torch.randint(0, 40, (n,), device="cuda"), greedy)
        return torch.div(c, 10, rounding_mode="floor").to(torch.uint8), (c % 10).to(torch.uint8)

    def kw(mode):
        state["draw"] += 1
        return dict(mode=mode, player=pt, seed=1, draw=state["draw"], epsilon=EPSILON, theta=1.0 if mode == "rank" else None)

    def kernel(mode):
        e = b.act_eval(te._ptr(ae), te._ptr(te.act_rot), te._ptr(te.act_trans), n_pieces=7, f16=dtype == torch.float16, mode=mode,
                       player=te._ptr(pt), seed=1, draw=7, epsilon=EPSILON, table=table_np if mode == "rank" else None)
        return lambda: b.select_eval_dev(e)

    te.select_eval(ae, **kw("argmax"))            # allocates the reused outputs
    paths = {}
    for mode in MODES:
        paths[f"torch_{mode}"] = lambda mode=mode: torch_choice(mode)
        paths[f"select_{mode}"] = lambda mode=mode: te.select_eval(ae, **kw(mode))
        paths[f"kernel_{mode}"] = kernel(mode)
    stepping = {}
    for mode in ("argmax", "pi"):
        stepping[f"torch_step_{mode}"] = lambda mode=mode: te.step_rt(*torch_choice(mode), player=pt, auto_reset=True)
        stepping[f"step_{mode}"] = lambda mode=mode: te.step_eval(ae, auto_reset=True, **kw(mode))
        stepping[f"torch_step_obs_{mode}"] = lambda mode=mode: te.step_rt_observe(*torch_choice(mode), player=pt, next_player=pt, auto_reset=True)
        stepping[f"step_obs_{mode}"] = lambda mode=mode: te.step_eval_observe(ae, next_player=pt, auto_reset=True, **kw(mode))
    # the same choice from both sides before anything is timed (argmax: no random numbers enter)
    r0, t0 = torch_choice("argmax")
    r1, t1 = te.select_eval(ae, **kw("argmax"))[:2]
    assert torch.equal(r0, r1) and torch.equal(t0, t1)
    out = {"clock_mhz": [b.clock_mhz()], "us_per_call": {}}
    for group in (paths, stepping):               # the paths that step the games last
        for fn in group.values():
            for _ in range(WARMUP):
                fn()
        torch.cuda.synchronize()
        windows = {name: [] for name in group}
        for _ in range(WINDOWS):
            for name, fn in group.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(CALLS):
                    fn()
                e1.record()
                e1.synchronize()
                windows[name].append(round(e0.elapsed_time(e1) * 1000.0 / CALLS, 2))
        for name, ws in windows.items():
            out["us_per_call"][name] = {"windows": ws, "median": statistics.median(ws), "min": min(ws), "max": max(ws)}
    out["clock_mhz"].append(b.clock_mhz())
    us = out["us_per_call"]
    nbytes = ae.numel() * ae.element_size()
    out["kernel_read_bandwidth"] = {name: {"bytes_read": nbytes, "us": us[name]["median"], "TB_per_s": round(nbytes / us[name]["median"] / 1e6, 3),
                                           "share_of_8_TB_per_s": round(nbytes / us[name]["median"] / 1e6 / (PEAK / 1e12), 3)}
                                    for name in us if name.startswith("kernel_")}

    def versus(new, old):
        a, o = us[new], us[old]
        return {"new": new, "old": old, "faster_in_every_window": all(x < y for x, y in zip(a["windows"], o["windows"])),
                "spreads_do_not_overlap": a["max"] < o["min"], "old_over_new": round(o["median"] / a["median"], 2)}

    out["acceptance"] = [versus(f"select_{m}", f"torch_{m}") for m in MODES]
    for m in ("argmax", "pi"):
        out["acceptance"] += [versus(f"step_{m}", f"torch_step_{m}"), versus(f"step_obs_{m}", f"torch_step_obs_{m}")]
    out["errors"] = b.take_errors()
    b.set_stream(None, external=False)
    b.close()
    return out


def main():
    dst = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "act")
    sizes = [int(v) for v in sys.argv[sys.argv.index("--sizes") + 1].split(",")] if "--sizes" in sys.argv else [4096, 16384, 65536]
    out = {"note": __doc__, "calls_per_window": CALLS, "cases": {}}
    for n in sizes:
        for P in (1, 2):
            for dtype_name in ("float32", "float16"):
                r = case(n, P, dtype_name)
                out["cases"][f"{n}_P{P}_{dtype_name}"] = r
                print(n, P, dtype_name, json.dumps({k: v["median"] for k, v in r["us_per_call"].items()}), flush=True)
                print("   ", json.dumps(r["acceptance"]), flush=True)
                os.makedirs(dst, exist_ok=True)
                with open(os.path.join(dst, "act_eval.json"), "w") as f:
                    json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
