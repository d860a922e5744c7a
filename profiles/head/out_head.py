"""Cost of the network's output heads: TorchEnv.q_head / policy_head (tetris_q_head_dev, tetris_policy_head_dev and their
_grad_dev) against the same expressions composed from torch ops (tests/head_support.py: the reference's lines), forward alone and
forward plus torch.autograd.grad with a dense incoming gradient.

    python profiles/head/out_head.py [--out DIR] [--sizes 4096,16384,65536] [--variant NAME=LIB ...]  -> DIR/out_head.json

M = 4 096, 16 384 and 65 536 samples, K = 7, Kv = 7, W = 8, float32 and float16 streams, the Q head in modes MEAN and MAX-joint with
the piece mask {0, 2, 5}, torch's stream.  Paths per case:
  torch_q_fwd / torch_q_fwd_bwd             the composition: amax / amin / mean / tanh and autograd.grad with respect to (a, v)
  q_fwd / q_fwd_bwd                         the library: one launch forward, one more backward
  torch_policy_fwd / .._bwd, policy_fwd / .._bwd   likewise for the policy head (once per size and element type)
A window = HIP events around 20 calls, nothing synchronised inside; five windows per path, all paths taken in turn within every
repeat, after a warm-up of each.  `bytes` is the traffic of the big arrays a path must move — forward 2 x 40 K M elements (read a,
write Q; A is not asked for), backward 3 x (read a and grad_Q, write grad_a) — the per-sample arrays, under 2 % of it, are left out;
`TB_per_s` is it over the median.  The outputs of both sides are compared before anything is timed.  --variant times the library
paths of another build of the library (another HEAD_BLOCK) at the largest size, in the same process, taken in turn with the
committed one."""
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import __graft_entry__ as ge  # noqa: E402
from tests.head_support import SOME, ref_action_softmax, ref_policy_value, ref_qva  # noqa: E402

CALLS, WINDOWS, WARMUP = 20, 5, 3
PEAK = 8.0e12
K = 7


def time_paths(torch, paths):
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
    return {name: {"windows": ws, "median": statistics.median(ws), "min": min(ws), "max": max(ws)} for name, ws in windows.items()}


def make_paths(torch, te, M, dtype, mode, policy=True, prefix=""):
    gen = torch.Generator(device="cuda").manual_seed(M)
    rand = lambda *s: torch.rand(*s, device="cuda", generator=gen)            # noqa: E731
    a = (4 * rand(M, 4, 10, K) - 2).to(dtype).requires_grad_()
    v = (2 * rand(M, K) - 1).to(dtype).requires_grad_()
    x = (8 * rand(M, 4, 10, K) - 4).to(dtype).requires_grad_()
    w = (2 * rand(M, K + 1) - 1).to(dtype).requires_grad_()
    G, gv = (2 * rand(M, 4, 10, K) - 1).to(dtype), (2 * rand(M, K) - 1).to(dtype)
    kw = dict(mode=mode, advantage_range=0.5, separate_piece_values=False, pieces=SOME)

    def torch_q():
        return ref_qva(v.reshape(M, 1, 1, K), a, 0.5, mode, False, SOME)

    def lib_q():
        return te.q_head(a, v, **kw)

    def no_grad(fn):
        def run():
            with torch.no_grad():
                return fn()
        return run

    def torch_policy():
        return ref_action_softmax(x), ref_policy_value(w, SOME, K)

    paths = {prefix + "q_fwd": no_grad(lib_q), prefix + "q_fwd_bwd": lambda: torch.autograd.grad(lib_q()[0], (a, v), G)}
    if not prefix:
        paths.update({"torch_q_fwd": no_grad(torch_q), "torch_q_fwd_bwd": lambda: torch.autograd.grad(torch_q()[0], (a, v), G)})
    if policy:
        paths.update({prefix + "policy_fwd": no_grad(lambda: te.policy_head(x, w)),
                      prefix + "policy_fwd_bwd": lambda: torch.autograd.grad(te.policy_head(x, w), (x, w), (G, gv))})
        if not prefix:
            paths.update({"torch_policy_fwd": no_grad(torch_policy), "torch_policy_fwd_bwd": lambda: torch.autograd.grad(torch_policy(), (x, w), (G, gv))})
    return paths


def same(torch, got, want, dtype, what):
    tol = 1e-2 if dtype == torch.float16 else 2e-5
    for g, t in zip(got, want):
        top = max(float(t.float().abs().max()), 1e-3)
        assert float((g.float() - t.float().reshape(g.shape)).abs().max()) <= tol * top, f"{what}: the two paths differ"


def case(M, dtype_name, mode, policy):
    import torch
    ti = importlib.import_module("drl-tetris_amd.torch_interop")
    pkg = ge.package()
    dtype = getattr(torch, dtype_name)
    b = pkg.TetrisBatch(8, 1, 20, 10, device=0)
    te = ti.TorchEnv(b)
    paths = make_paths(torch, te, M, dtype, mode, policy)
    for head in ("q", "policy") if policy else ("q",):
        same(torch, [t.clone() for t in paths[head + "_fwd"]()[:2]], paths[f"torch_{head}_fwd"]()[:2], dtype, head + " forward")
        same(torch, [t.clone() for t in paths[head + "_fwd_bwd"]()], paths[f"torch_{head}_fwd_bwd"](), dtype, head + " backward")
    out = {"clock_mhz": [b.clock_mhz()]}
    us = out["us_per_call"] = time_paths(torch, paths)
    out["clock_mhz"].append(b.clock_mhz())
    one = M * 40 * K * (2 if dtype == torch.float16 else 4)
    out["head_bandwidth"] = {}
    for name in paths:
        if not name.startswith("torch_"):
            nbytes = one * (5 if name.endswith("_bwd") else 2)
            out["head_bandwidth"][name] = {"bytes": nbytes, "us": us[name]["median"], "TB_per_s": round(nbytes / us[name]["median"] / 1e6, 3),
                                           "share_of_8_TB_per_s": round(nbytes / us[name]["median"] / 1e6 / (PEAK / 1e12), 3)}

    def versus(new, old_name):
        n_, o_ = us[new], us[old_name]
        return {"new": new, "old": old_name, "faster_in_every_window": all(x < y for x, y in zip(n_["windows"], o_["windows"])),
                "spreads_do_not_overlap": n_["max"] < o_["min"], "old_over_new": round(o_["median"] / n_["median"], 2)}

    out["versus_torch"] = [versus(n, "torch_" + n) for n in paths if not n.startswith("torch_")]
    out["errors"] = b.take_errors()
    b.set_stream(None, external=False)
    b.close()
    return out


def variants(M, dtype_name, libs):
    """the library paths of the committed build and of other builds, taken in turn"""
    import torch
    ti = importlib.import_module("drl-tetris_amd.torch_interop")
    pkg = ge.package()
    dtype = getattr(torch, dtype_name)
    paths, batches = {}, []
    for name, lib in [("block16", None)] + libs:
        b = pkg.TetrisBatch(8, 1, 20, 10, device=0, **({"lib_path": lib} if lib else {}))
        batches.append(b)
        paths.update(make_paths(torch, ti.TorchEnv(b), M, dtype, "mean", True, prefix=name + "_"))
    us = time_paths(torch, paths)
    for b in batches:
        b.set_stream(None, external=False)
        b.close()
    return us


def main():
    arg = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default          # noqa: E731
    dst = arg("--out", os.path.join(ROOT, "profiles", "head"))
    sizes = [int(x) for x in arg("--sizes", "4096,16384,65536").split(",")]
    libs = [tuple(sys.argv[i + 1].split("=", 1)) for i, t in enumerate(sys.argv) if t == "--variant"]
    out = {"note": __doc__, "calls_per_window": CALLS, "cases": {}}

    def save():
        os.makedirs(dst, exist_ok=True)
        with open(os.path.join(dst, "out_head.json"), "w") as f:
            json.dump(out, f, indent=1)
    for M in sizes:
        for dtype_name in ("float32", "float16"):
            for mode in ("mean", "max"):
                r = case(M, dtype_name, mode, policy=mode == "mean")
                out["cases"][f"{M}_{dtype_name}_{mode if mode == 'mean' else 'max_joint'}"] = r
                print(M, dtype_name, mode, json.dumps({k: x["median"] for k, x in r["us_per_call"].items()}), flush=True)
                print("   ", json.dumps(r["versus_torch"]), flush=True)
                save()
    if libs:
        out["block_variants"] = {}
        for dtype_name in ("float32", "float16"):
            us = out["block_variants"][f"{sizes[-1]}_{dtype_name}_mean"] = variants(sizes[-1], dtype_name, libs)
            print("variants", dtype_name, json.dumps({k: x["median"] for k, x in us.items()}), flush=True)
            save()


if __name__ == "__main__":
    main()
