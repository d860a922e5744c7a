"""Cost of the trainer's loss heads: TorchEnv.ppo_head / dqn_head (tetris_ppo_loss_dev, tetris_dqn_loss_dev) against the same
loss composed from torch ops, forward plus torch.autograd.grad with respect to pi and v / Q.

    python profiles/loss/loss_head.py [--out DIR] [--sizes 4096,16384,65536]    -> DIR/loss_head.json (default profiles/loss)

M = 4 096, 16 384 and 65 536 samples, K = 7, V = 7, float32 and float16 network outputs, a valid mask and (DQN) importance
weights, torch's stream.  Paths:
  torch_ppo / torch_dqn   the composition: a gather of the piece's plane, the element-wise formulas, autograd.grad
  ppo_head / dqn_head     the library call (a count launch, the head, the reduction of the statistics)
A window = HIP events around 20 calls, nothing synchronised inside; five windows per path, both paths of a head taken in turn
within every repeat, after a warm-up of each.  Per call the head reads 40 K elements per sample and writes 40 K: `bytes` is that
traffic (the per-sample arrays, under 1 % of it, are left out), `TB_per_s` it over the median.  The gradients of both paths are
compared before anything is timed.  Reported per path: the windows, their median, lowest and highest (us per call)."""
import importlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import __graft_entry__ as ge  # noqa: E402

CALLS, WINDOWS, WARMUP = 20, 5, 3
PEAK = 8.0e12
PRM = dict(clipping_parameter=0.15, value_loss=0.3, policy_loss=1.0, entropy_loss=0.01, ppo_epsilon=0.9, entropy_floor_loss=1.0, rescaled_entropy=0.5)


def case(M, dtype_name):
    import torch
    ti = importlib.import_module("drl-tetris_amd.torch_interop")
    pkg = ge.package()
    dtype = getattr(torch, dtype_name)
    b = pkg.TetrisBatch(8, 1, 20, 10, device=0)
    te = ti.TorchEnv(b)
    K = 7
    gen = torch.Generator(device="cuda").manual_seed(M)
    rand = lambda *s: torch.rand(*s, device="cuda", generator=gen)            # noqa: E731
    raw = rand(M, 4, 10, K) ** 3 + 1e-6
    pi = (raw / raw.sum(dim=(1, 2), keepdim=True)).to(dtype).contiguous()
    v = (rand(M, K) - 0.5).to(dtype).contiguous()
    Q = (rand(M, 4, 10, K) - 0.5).to(dtype).contiguous()
    action = torch.stack([torch.randint(0, 4, (M,), device="cuda", generator=gen), torch.randint(0, 10, (M,), device="cuda", generator=gen),
                          torch.randint(0, K, (M,), device="cuda", generator=gen)], dim=1).to(torch.uint8).contiguous()
    rows, a = torch.arange(M, device="cuda"), action.long()
    c = 10 * a[:, 0] + a[:, 1]
    old = (pi.view(M, 40, K)[rows, c, a[:, 2]].float() / (0.5 + 1.5 * rand(M))).contiguous()
    adv, target, weight = rand(M) - 0.5, rand(M) - 0.5, rand(M).contiguous()
    valid = (rand(M) > 0.05).to(torch.uint8)
    floor, hmax = pkg.capi.ppo_entropy_constants(PRM["ppo_epsilon"])
    sel = valid != 0

    def torch_ppo():
        p_, v_ = pi.detach().requires_grad_(), v.detach().requires_grad_()
        plane = p_.view(M, 40, K)[rows, :, a[:, 2]].float()
        prob = plane[rows, c]
        val = v_[rows, a[:, 2]].float()
        r = torch.clamp(prob, min=1e-6) / torch.clamp(old, min=1e-6)
        pl = torch.minimum(r * adv, torch.clamp(r, 1 - PRM["clipping_parameter"], 1 + PRM["clipping_parameter"]) * adv)
        q = plane + 1e-6
        H = -(q * torch.log(torch.clamp(q, min=1e-6))).sum(dim=1)
        bonus = H - PRM["entropy_floor_loss"] * torch.relu(floor - H)
        bonus = bonus + PRM["rescaled_entropy"] * (hmax - bonus)
        loss = (PRM["value_loss"] * ((val - target) ** 2)[sel].mean() - PRM["policy_loss"] * pl[sel].mean() - PRM["entropy_loss"] * bonus[sel].mean())
        return (loss.detach(),) + torch.autograd.grad(loss, (p_, v_))

    def torch_dqn():
        q_ = Q.detach().requires_grad_()
        q = q_.view(M, 40, K)[rows, c, a[:, 2]].float()
        w = weight * sel
        loss = (w * (q - target) ** 2).sum() / (w != 0).sum()
        return loss.detach(), torch.autograd.grad(loss, q_)[0], (q - target).abs().detach()

    paths = {"torch_ppo": torch_ppo, "ppo_head": lambda: te.ppo_head(pi, v, action, old, adv, target, valid, **PRM),
             "torch_dqn": torch_dqn, "dqn_head": lambda: te.dqn_head(Q, action, target, weight, valid)}
    # the same gradients from both sides before anything is timed
    tl, tg_pi, tg_v = torch_ppo()
    stats, g_pi, g_v = te.ppo_head(pi, v, action, old, adv, target, valid, **PRM)
    tol = 2e-3 if dtype == torch.float16 else 1e-5
    top = float(tg_pi.float().abs().max())
    assert float((g_pi.float() - tg_pi.float()).abs().max()) <= tol * top + (6e-8 if dtype == torch.float16 else 0.0), "grad_pi of the two paths differs"
    assert float((g_v.float() - tg_v.float()).abs().max()) <= tol * float(tg_v.float().abs().max()) + (6e-8 if dtype == torch.float16 else 0.0)
    assert abs(float(stats[1]) - float(tl)) <= 1e-4 * max(1.0, abs(float(tl)))
    tl, tg_q, _ = torch_dqn()
    stats, g_q, _, _ = te.dqn_head(Q, action, target, weight, valid)
    assert float((g_q.float() - tg_q.float()).abs().max()) <= tol * float(tg_q.float().abs().max()) + (6e-8 if dtype == torch.float16 else 0.0)
    assert abs(float(stats[2]) - float(tl)) <= 1e-4 * max(1.0, abs(float(tl)))
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
    for name, ws in windows.items():
        out["us_per_call"][name] = {"windows": ws, "median": statistics.median(ws), "min": min(ws), "max": max(ws)}
    out["clock_mhz"].append(b.clock_mhz())
    us = out["us_per_call"]
    nbytes = 2 * pi.numel() * pi.element_size()
    out["head_bandwidth"] = {name: {"bytes": nbytes, "us": us[name]["median"], "TB_per_s": round(nbytes / us[name]["median"] / 1e6, 3),
                                    "share_of_8_TB_per_s": round(nbytes / us[name]["median"] / 1e6 / (PEAK / 1e12), 3)}
                             for name in ("ppo_head", "dqn_head")}

    def versus(new, old_name):
        n_, o_ = us[new], us[old_name]
        return {"new": new, "old": old_name, "faster_in_every_window": all(x < y for x, y in zip(n_["windows"], o_["windows"])),
                "spreads_do_not_overlap": n_["max"] < o_["min"], "old_over_new": round(o_["median"] / n_["median"], 2)}

    out["acceptance"] = [versus("ppo_head", "torch_ppo"), versus("dqn_head", "torch_dqn")]
    out["errors"] = b.take_errors()
    b.set_stream(None, external=False)
    b.close()
    return out


def main():
    dst = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "loss")
    sizes = [int(x) for x in sys.argv[sys.argv.index("--sizes") + 1].split(",")] if "--sizes" in sys.argv else [4096, 16384, 65536]
    out = {"note": __doc__, "calls_per_window": CALLS, "cases": {}}
    for M in sizes:
        for dtype_name in ("float32", "float16"):
            r = case(M, dtype_name)
            out["cases"][f"{M}_{dtype_name}"] = r
            print(M, dtype_name, json.dumps({k: x["median"] for k, x in r["us_per_call"].items()}), flush=True)
            print("   ", json.dumps(r["acceptance"]), json.dumps(r["head_bandwidth"]), flush=True)
            os.makedirs(dst, exist_ok=True)
            with open(os.path.join(dst, "loss_head.json"), "w") as f:
                json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
