"""Cost of a planning agent's decision between the network and the step: the library call (tetris_select_lists_dev through
TorchEnv.choose_lists) against the same decision composed from torch ops on the entry points the library had before it.

    python profiles/plan/plan_choose.py [--out DIR] [--sizes 4096,16384]    -> DIR/plan_choose.json (default profiles/plan)

20x10 two-player games after 18 random steps, 64 lists of 48 keys, K = 7, strictly positive phi, torch's stream; 4 096 and 16 384
games, phi in float32 and float16 (the planes and the composition's deltas in the same type), both modes.  Paths:
  simulate         TorchEnv.simulate(finalize=False) alone: both sides below begin with it
  torch_<mode>     TorchEnv.deltas() (simulate + tetris_plan_deltas_dev), the gather of the piece's phi plane (the piece index
                   comes from one observe() before the windows, as an agent has it from before its network ran), (deltas *
                   phi_p).sum((1, 2)), the normalisation, argmax / torch.multinomial, the gather of the chosen plane
  choose_<mode>    TorchEnv.choose_lists (simulate + tetris_select_lists_dev)
  kernel_<mode>    tetris_select_lists_dev alone over a prepared argument struct
A window = HIP events around 20 calls, nothing synchronised inside; five windows per path, the paths taken in turn within every
repeat, after a warm-up of every path.  The shader clock (tetris_debug_clock_khz) is read before and after each case.  Reported per
path: the windows, their median, lowest and highest (us per call); per case the bytes each side has to move, from the shapes
(arithmetic, not a counter): the composition writes the deltas [N, H, 10, L] and reads them again for the product; the call
reads the acting players' column words [N, L, 10] twice (scores, then the sums' counts: the second time from L2), one phi plane
in K and writes two [N, H, 10] planes.  `acceptance` states for every pair whether the new call was faster in every window."""
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
MODES = ("argmax", "pi")
L, K, H = 64, 7, 20


def bytes_moved(n, esize):
    deltas = n * H * 10 * L * esize
    phi = n * H * 10 * K * esize
    return {"torch": {"deltas_written": deltas, "deltas_read_by_the_product": deltas, "phi_gathered_lines": phi, "products_written_and_reduced": 2 * deltas,
                      "chosen_plane_gather": 2 * n * H * 10 * esize},
            "choose": {"column_words_of_the_acting_player_read_twice": 2 * n * L * 10 * 4, "phi_lines": phi, "two_planes_written": 2 * n * H * 10 * esize}}


def case(n, dtype_name):
    import torch
    ti = importlib.import_module("drl-tetris_amd.torch_interop")
    pkg = ge.package()
    dtype = getattr(torch, dtype_name)
    b = pkg.TetrisBatch(n, 2, H, 10, seeds=orc.episode_seed(np.arange(n), 0), device=0)
    b.rollout_random(1, 18)
    te = ti.TorchEnv(b)
    gen = torch.Generator(device="cuda").manual_seed(0)
    pt = (torch.arange(n, device="cuda") % 2).to(torch.uint8)
    phi = (torch.rand(n, H, 10, K, device="cuda", generator=gen) + 0.1).to(dtype).contiguous()
    rows = torch.arange(n, device="cuda")
    te.action_lists(player=pt, max_lists=L)
    state = {"draw": 0}

    piece = te.observe(pt)[2][0].clone()          # (an agent has observed before it ran its network: outside the windows)

    def torch_choice(mode):
        d, s = te.deltas(player=pt, dtype=dtype)
        phi_p = phi[rows, :, :, piece.long()]
        score = (d * phi_p.unsqueeze(-1)).sum(dim=(1, 2)).float()
        probs = score / score.sum(dim=1, keepdim=True)
        c = probs.argmax(dim=1) if mode == "argmax" else torch.multinomial(probs.clamp_min(0.0), 1).squeeze(1)
        return c.to(torch.int32), probs[rows, c], d[rows, :, :, c], s

    def choose(mode):
        state["draw"] += 1
        return te.choose_lists(phi, mode=mode, player=pt, seed=1, draw=state["draw"], out_dtype=dtype)

    def kernel(mode):
        cols = te.simulate(pt, finalize=False)[0]
        out = dict(choice=torch.zeros(n, dtype=torch.int32, device="cuda"), piece=torch.zeros(n, dtype=torch.uint8, device="cuda"),
                   prob=torch.zeros(n, device="cuda"), entropy=torch.zeros(n, device="cuda"),
                   delta=torch.zeros(n, H, 10, dtype=dtype, device="cuda"), sums=torch.zeros(n, H, 10, dtype=dtype, device="cuda"))
        e = b.plan_eval(te._ptr(phi), te._ptr(te.list_count), te._ptr(cols), te._ptr(out["choice"]), n_pieces=K, f16=dtype == torch.float16,
                        mode=mode, player=te._ptr(pt), seed=1, draw=7, max_lists=L, out_f16=dtype == torch.float16, piece=te._ptr(out["piece"]),
                        prob=te._ptr(out["prob"]), entropy=te._ptr(out["entropy"]) if mode == "pi" else None, delta=te._ptr(out["delta"]),
                        sums=te._ptr(out["sums"]))
        return lambda e=e, out=out: b.select_lists_dev(e)          # (the struct and its tensors live with the path)

    paths = {"simulate": lambda: te.simulate(pt, finalize=False)}
    for mode in MODES:
        paths[f"torch_{mode}"] = lambda mode=mode: torch_choice(mode)
        paths[f"choose_{mode}"] = lambda mode=mode: choose(mode)
        paths[f"kernel_{mode}"] = kernel(mode)
    # the same planes from both sides before anything is timed, and the same choice wherever the composition's two best differ
    c0, p0, d0, s0 = torch_choice("argmax")
    c1, _, p1, _, _, d1, s1 = choose("argmax")
    assert torch.equal(s1, s0[..., 0])
    same = c0 == c1
    assert torch.equal(d1[same], d0[same]) and (dtype == torch.float16 or same.float().mean().item() > 0.95)
    out = {"clock_mhz": [b.clock_mhz()], "us_per_call": {}, "choices_equal_share": round(same.float().mean().item(), 4)}
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
    out["bytes_moved"] = bytes_moved(n, phi.element_size())

    def versus(new, old):
        a, o = us[new], us[old]
        return {"new": new, "old": old, "faster_in_every_window": all(x < y for x, y in zip(a["windows"], o["windows"])),
                "spreads_do_not_overlap": a["max"] < o["min"], "old_over_new": round(o["median"] / a["median"], 2)}

    out["acceptance"] = [versus(f"choose_{m}", f"torch_{m}") for m in MODES]
    out["errors"] = b.take_errors()
    b.set_stream(None, external=False)
    b.close()
    return out


def main():
    dst = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "plan")
    sizes = [int(v) for v in sys.argv[sys.argv.index("--sizes") + 1].split(",")] if "--sizes" in sys.argv else [4096, 16384]
    out = {"note": __doc__, "calls_per_window": CALLS, "cases": {}}
    for n in sizes:
        for dtype_name in ("float32", "float16"):
            r = case(n, dtype_name)
            out["cases"][f"{n}_{dtype_name}"] = r
            print(n, dtype_name, json.dumps({k: v["median"] for k, v in r["us_per_call"].items()}), flush=True)
            print("   ", json.dumps(r["acceptance"]), flush=True)
            os.makedirs(dst, exist_ok=True)
            with open(os.path.join(dst, "plan_choose.json"), "w") as f:
                json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
