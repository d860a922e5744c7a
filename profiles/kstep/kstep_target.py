"""Cost of the k-step target estimator and of the step-list gather: Replay.targets (tetris_kstep_target_dev, ring mode) against the
same target composed from torch ops on the same tensors, and Replay.gather with a step list (tetris_replay_gather_steps_dev)
against the full k + 1 gather.

    python profiles/kstep/kstep_target.py [--out DIR] [--sizes 4096,16384,65536]    -> DIR/kstep_target.json (default profiles/kstep)

M = 4 096, 16 384 and 65 536 samples; k = 5 and 37, each with all steps and with filter [2, 3]; K = 7, all pieces used; float32
and float16 outputs of the net; Q mode (Q [M n, 4, 10, 7]) and V mode (v [M n, 7]); torch's stream.  Paths:
  torch_target   the composition: amax over (r, t), the masked mean, an index_select of the reward and done rows from the ring,
                 cumsum for the done time, the loop over the k steps, the division
  targets        the library call (Q mode: the values launch and the estimator launch; V mode: the estimator launch)
  gather_full / gather_list   the gather of steps 0..k against the gather of the step list, visual and vector included
A window = HIP events around 20 calls, nothing synchronised inside; five windows per path, the paths taken in turn within every
repeat, after a warm-up of each.  `bytes` of a targets call is the net's output, read once (the per-sample arrays and the values,
under 1 % of it in Q mode, are left out); `TB_per_s` it over the median.  The targets of both paths are compared before anything is
timed.  Reported per path: the windows, their median, lowest and highest (us per call)."""
import importlib
import json
import os
import statistics
import sys

import numpy as np

ROOT =os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import __graft_entry__ as ge  # noqa: E402

CALLS, WINDOWS, WARMUP = 20, 5, 3
PEAK = 8.0e12
GAMMA, LAM = 0.99, 0.9


def case(M, k, steps, dtype_name, values):
    import torch
    ti = importlib.import_module("drl-tetris_amd.torch_interop")
    pkg = ge.package()
    dtype = getattr(torch, dtype_name)
    b = pkg.TetrisBatch(8, 1, 20, 10, device=0)
    te = ti.TorchEnv(b)
    K, n = 7, len(steps)
    gen = torch.Generator(device="cuda").manual_seed(M + k)
    rand = lambda *s: torch.rand(*s, device="cuda", generator=gen)            # noqa: E731
    max_size = 1 << 18
    rp = te.replay(max_size + k, k_step=k)
    rp.reward[:max_size] = 2 * rand(max_size) - 1
    rp.done[:max_size] = (rand(max_size) < 1.0 / (k + 1)).to(torch.uint8)
    rp.obs[:max_size] = torch.randint(0, 1 << 20, tuple(rp.obs[:max_size].shape), device="cuda", generator=gen, dtype=torch.int32)
    rp.flags[:max_size] = (rand(max_size) < 0.5).to(torch.uint8)
    index = torch.randint(0, max_size, (M,), device="cuda", generator=gen, dtype=torch.int32)
    out = ((2 * rand(M * n, K) - 1) if values else (2 * rand(M * n, 4, 10, K) - 1)).to(dtype).contiguous()
    g =[float(np.float32(float(np.float32(GAMMA)) ** t)) for t in range(k + 1)]
    l = [float(np.float32(float(np.float32(LAM)) ** t)) for t in range(k + 1)]
    offs = torch.arange(k + 1, device="cuda")
    step_set = set(steps)

    def torch_target():
        if values:
            V = out.view(M, n, K).float().sum(dim=2) / K
        else:
            V = out.view(M, n, 40, K).amax(dim=2).float().sum(dim=2) / K
        at = (index.long()[:, None] + offs[None, :]).reshape(-1)
        r = torch.index_select(rp.reward, 0, at).view(M, k + 1)
        d = (torch.index_select(rp.done, 0, at).view(M, k + 1) != 0).float()
        dt = (1 - torch.cumsum(d, dim=1).clamp(max=1)).sum(dim=1)
        P, num, den, i = 0, 0, 0, 0
        for s in range(1, k + 1):
            P = P + r[:, s - 1] * (dt >= s - 1) * g[s - 1]
            if s in step_set:
                E = P + V[:, i] * (dt >= s) * g[s]
                num = num + E * l[s]
                den = den + l[s]
                i += 1
        return num / den

    paths = {"torch_target": torch_target,
             "targets": lambda: rp.targets(index, out, steps=steps, gamma=GAMMA, lam=LAM, values=values)}
    if not values and dtype == torch.float32:
        paths["gather_full"] = lambda: rp.gather(index, steps=k + 1)
        paths["gather_list"] = lambda: rp.gather(index, steps=steps)
    want, got = torch_target(), paths["targets"]().clone()
    torch.cuda.synchronize()
    worst = float((want - got).abs().max())
    assert worst <= 1e-4 * (k + 1), f"the two paths differ by {worst}"
    res = {"M": M, "k": k, "n": n, "dtype": dtype_name, "mode": "V" if values else "Q", "largest_difference": worst,
           "clock_mhz": [b.clock_mhz()], "us_per_call": {}}
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
    us = res["us_per_call"]
    for name, ws in windows.items():
        us[name] = {"windows": ws, "median": statistics.median(ws), "min": min(ws), "max": max(ws)}
    res["clock_mhz"].append(b.clock_mhz())
    nbytes = out.numel() * out.element_size()
    res["bandwidth"] = {"bytes": nbytes, "us": us["targets"]["median"], "TB_per_s": round(nbytes / us["targets"]["median"] / 1e6, 3),
                        "share_of_8_TB_per_s": round(nbytes / us["targets"]["median"] / 1e6 / (PEAK / 1e12), 3)}

    def versus(new, old_name):
        n_, o_ = us[new], us[old_name]
        return {"new": new, "old": old_name, "faster_in_every_window": all(x < y for x, y in zip(n_["windows"], o_["windows"])),
                "spreads_do_not_overlap": n_["max"] < o_["min"], "old_over_new": round(o_["median"] / n_["median"], 2)}

    res["comparison"] = [versus("targets", "torch_target")] + ([versus("gather_list", "gather_full")] if "gather_list" in paths else [])
    res["errors"] = b.take_errors()
    b.set_stream(None, external=False)
    b.close()
    del rp, out
    torch.cuda.empty_cache()
    return res


def main():
    pkg = ge.package()
    dst = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "kstep")
    sizes = [int(x) for x in sys.argv[sys.argv.index("--sizes") + 1].split(",")] if "--sizes" in sys.argv else [4096, 16384, 65536]
    result = {"note": __doc__, "calls_per_window": CALLS, "cases": {}}
    for M in sizes:
        for k in (5, 37):
            for name, steps in (("all", pkg.capi.kstep_steps(k)), ("filter23", pkg.capi.kstep_steps(k, [2, 3]))):
                for dtype_name in ("float32", "float16"):
                    for values in (False, True):
                        r = case(M, k, steps, dtype_name, values)
                        result["cases"][f"{M}_k{k}_{name}_{dtype_name}_{'V' if values else 'Q'}"] = r
                        print(M, k, name, dtype_name, "V" if values else "Q", json.dumps({p: x["median"] for p, x in r["us_per_call"].items()}),
                              json.dumps(r["comparison"]), json.dumps(r["bandwidth"]), flush=True)
                        os.makedirs(dst, exist_ok=True)
                        with open(os.path.join(dst, "kstep_target.json"), "w") as f:
                            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
