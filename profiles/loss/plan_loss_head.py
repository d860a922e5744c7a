"""Cost of the planning loss head: TorchEnv.plan_head (tetris_plan_loss_dev) against the same loss composed from
Trajectory.batch_plan plus torch ops, forward plus torch.autograd.grad with respect to phi and v — what a user of the planning
path runs without the head.

    python profiles/loss/plan_loss_head.py [--out DIR] [--sizes 4096,16384,65536]    -> DIR/plan_loss_head.json (default profiles/loss)

M = 4 096, 16 384 and 65 536 samples, H = 20, K = V = 7, float32 and float16 network outputs, a valid mask, half the indices
mirrored, small_fill = 0, torch's stream.  The window: 4 096 two-player games after 18 random steps, four recorded rows of up to
64 lists (16 384 entries); the index list draws from them with repeats.  Paths:
  torch_plan   batch_plan(index) (two float32 [M, 20, 10] planes), the piece's plane of clip(phi), the element-wise formulas of
               delta_ppo_nets.py:150-182, autograd.grad
  plan_head    the library call (a count launch, the head, the reduction of the statistics)
A window = HIP events around 20 calls, nothing synchronised inside; five windows per path, the two paths taken in turn within
every repeat, after a warm-up of each.  Per call the head reads H 10 K elements per sample and a 448-byte record and writes H 10 K
elements: `bytes` is that traffic (the per-sample arrays, under 1 % of it, are left out), `TB_per_s` it over the median.  The
gradients of both paths are compared before anything is timed.  Reported per path: the windows, their median, lowest and highest
(us per call)."""
import importlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import __graft_entry__ as ge  # noqa: E402
from oracle import oracle as orc  # noqa: E402

CALLS, WINDOWS, WARMUP = 20, 5, 3
PEAK = 8.0e12
N, T, L, H, K = 4096, 4, 64, 20, 7
PRM = dict(clipping_parameter=0.15, value_loss=0.3, policy_loss=1.0, entropy_loss=0.01, impossibility_loss=0.1)


def window():
    import torch
    ti = importlib.import_module("drl-tetris_amd.torch_interop")
    b = ge.package().TetrisBatch(N, 2, H, 10, seeds=orc.episode_seed(np.arange(N), 2), device=0)
    b.rollout_random(1, 18)
    te = ti.TorchEnv(b)
    tr = te.trajectory(T, states=True, plan=True)
    gen = torch.Generator(device="cuda").manual_seed(1)
    for t in range(T):
        pt = ((torch.arange(N, device="cuda") + t) % 2).to(torch.uint8)
        te.action_lists(player=pt, max_lists=L)
        tr.observe(t, pt)
        te.step_lists_eval(torch.rand(N, H, 10, K, generator=gen, device="cuda") + 0.1, mode="pi", player=pt, seed=3, draw=t, auto_reset=True, planes=False)
        tr.record_plan(t)
    return b, te, tr


def case(b, te, tr, M, dtype_name):
    import torch
    dtype = getattr(torch, dtype_name)
    gen = torch.Generator(device="cuda").manual_seed(M)
    rand = lambda *s: torch.rand(*s, device="cuda", generator=gen)            # noqa: E731
    phi = (1.2 * rand(M, H, 10, K) - 0.05).to(dtype).contiguous()             # below e, inside and above 1
    v = (rand(M, K) - 0.5).to(dtype).contiguous()
    index = torch.randint(0, T * N, (M,), device="cuda", generator=gen, dtype=torch.int64)
    index = torch.where(torch.arange(M, device="cuda") % 2 == 1, index | (1 << 31), index).to(torch.int32)
    action = torch.stack([torch.zeros(M, device="cuda"), torch.zeros(M, device="cuda"), torch.randint(0, K, (M,), device="cuda", generator=gen)],
                         dim=1).to(torch.uint8).contiguous()
    piece = action[:, 2]
    rows, k = torch.arange(M, device="cuda"), piece.long()
    adv, target = rand(M) - 0.5, rand(M) - 0.5
    valid = (rand(M) > 0.05).to(torch.uint8)
    sel = valid != 0
    e, clip = 1e-6, PRM["clipping_parameter"]
    stats, _, _, terms = te.plan_head(phi, v, tr, index, piece, torch.ones(M, device="cuda"), adv, target, valid, small_fill=0.0, terms=True, **PRM)
    old = (terms[0].clamp(min=1e-3) / (0.5 + 1.5 * rand(M))).contiguous()

    def torch_plan():
        p_, v_ = phi.detach().requires_grad_(), v.detach().requires_grad_()
        planes = tr.batch_plan(index, small_fill=0.0)
        x = torch.clamp(p_[rows, :, :, k].float(), e, 1.0)[..., None]            # (the piece's plane first: the cheapest order)
        val = v_[rows, k].float()
        probability = ((x * planes.delta).sum(dim=(1, 2, 3)) + e) / ((x * planes.sums).sum(dim=(1, 2, 3)) + e)
        r = torch.clamp(probability, min=e) / torch.clamp(old, min=e)
        pl = torch.minimum(r * adv, torch.clamp(r, 1 - clip, 1 + clip) * adv)
        imp = x * (1 - torch.clamp(planes.sums, max=1.0))
        y = x * planes.sums / (planes.sums + e).sum(dim=(1, 2, 3), keepdim=True) + e
        Hent = -(y * torch.log(torch.clamp(y, min=e))).sum(dim=(1, 2, 3))
        loss = (PRM["value_loss"] * ((val - target) ** 2)[sel].mean() - PRM["policy_loss"] * pl[sel].mean()
                + PRM["impossibility_loss"] * imp[sel].mean() - PRM["entropy_loss"] * Hent[sel].mean())
        return (loss.detach(),) + torch.autograd.grad(loss, (p_, v_))

    paths = {"torch_plan": torch_plan,
             "plan_head": lambda: te.plan_head(phi, v, tr, index, piece, old, adv, target, valid, small_fill=0.0, **PRM)}
    # the same gradients from both sides before anything is timed
    tl, tg_phi, tg_v = torch_plan()
    stats, g_phi, g_v = te.plan_head(phi, v, tr, index, piece, old, adv, target, valid, small_fill=0.0, **PRM)
    tol = 2e-3 if dtype == torch.float16 else 1e-4
    floor = 6e-8 if dtype == torch.float16 else 0.0
    top = float(tg_phi.float().abs().max())
    diff = float((g_phi.float() - tg_phi.float()).abs().max())
    assert diff <= tol * top + floor, f"grad_phi of the two paths differs: {diff} of {top}"
    assert float((g_v.float() - tg_v.float()).abs().max()) <= tol * float(tg_v.float().abs().max()) + floor
    assert abs(float(stats[1]) - float(tl)) <= 1e-4 * max(1.0, abs(float(tl)))
    out = {"clock_mhz": [b.clock_mhz()], "us_per_call": {}, "grad_phi_largest": top, "grad_phi_largest_difference": diff}
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
    nbytes = 2 * phi.numel() * phi.element_size() + 448 * M
    med = us["plan_head"]["median"]
    out["head_bandwidth"] = {"bytes": nbytes, "us": med, "TB_per_s": round(nbytes / med / 1e6, 3), "share_of_8_TB_per_s": round(nbytes / med / 1e6 / (PEAK / 1e12), 3)}
    n_, o_ = us["plan_head"], us["torch_plan"]
    out["acceptance"] = {"new": "plan_head", "old": "torch_plan", "faster_in_every_window": all(x < y for x, y in zip(n_["windows"], o_["windows"])),
                         "spreads_do_not_overlap": n_["max"] < o_["min"], "old_over_new": round(o_["median"] / n_["median"], 2)}
    out["errors"] = b.take_errors()
    return out


def main():
    import torch
    dst = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "loss")
    sizes = [int(x) for x in sys.argv[sys.argv.index("--sizes") + 1].split(",")] if "--sizes" in sys.argv else [4096, 16384, 65536]
    out = {"note": __doc__, "calls_per_window": CALLS, "cases": {}}
    b, te, tr = window()
    for M in sizes:
        for dtype_name in ("float32", "float16"):
            r = case(b, te, tr, M, dtype_name)
            out["cases"][f"{M}_{dtype_name}"] = r
            print(M, dtype_name, json.dumps({k: x["median"] for k, x in r["us_per_call"].items()}), json.dumps(r["acceptance"]), json.dumps(r["head_bandwidth"]), flush=True)
            os.makedirs(dst, exist_ok=True)
            with open(os.path.join(dst, "plan_loss_head.json"), "w") as f:
                json.dump(out, f, indent=1)
    torch.cuda.synchronize()
    b.set_stream(None, external=False)
    b.close()


if __name__ == "__main__":
    main()
