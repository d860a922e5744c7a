"""Cost of one residual layer: TorchEnv.residual_layer (tetris_res_layer_dev and its _grad_x_dev / _grad_w_dev) against the same layer
composed from torch ops on the same tensors — F.conv2d(padding=1), the join, F.elu (tests/res_support.py: ref_residual_layer) —,
forward under no_grad and forward plus torch.autograd.grad with a dense incoming gradient; and the three-layer block against the
same block from torch ops.

    python profiles/res/res_layer.py [--out DIR] [--sizes 1024,4096,16384]          -> DIR/res_layer.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o res -- python profiles/res/res_layer.py --kernels     (a run of its own)
    python profiles/res/res_layer.py --out DIR --stats DIR/res_kernel_stats.csv      -> adds "kernels" to the json

Hp = 22, Ci = Co = 128, ADD + ELU, float32 and float16, M = 1 024, 4 096 and 16 384, once with a channels_last input and once with
a channels-first one on both sides, so that the layout copy is counted where it occurs (the library's wrapper copies; torch's
conv2d chooses for itself); one case with Ci = 136; the block at the middle size.  kbd_conv.py's method: a window = HIP events around
20 calls, nothing synchronised inside; five windows per path, the paths of a case taken in turn within every repeat, after a warm-up
of every path of every case (torch's convolution picks its algorithm on first use).  The clock is noted before and after a case.
The outputs of both sides are compared before anything is timed.
--kernels runs ten calls of each entry point through capi at M = 16 384 for a kernel trace; --stats reads the trace's kernel
statistics and sets each kernel's average time against the larger of its bytes over 8 TB/s and its operations over the matrix
peak (2 516.8 TFLOP/s binary16, 157.3 float32), both computed from the shapes by bounds() below, and says which applies."""
import csv
import ctypes as C
import importlib
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import __graft_entry__ as ge  # noqa: E402
from tests.res_support import ref_residual_layer  # noqa: E402

CALLS, WINDOWS, WARMUP = 20, 5, 3
HBM, PEAK = 8.0e12, {"float16": 2516.8e12, "float32": 157.3e12}
HP, CH = 22, 128
ROWS, W_SAMPLES = 8, 64          # tetris_res.h: RES_ROWS, RES_W_SAMPLES


def bounds(M, dtype_name, Ci=CH, Co=CH):
    """per kernel (ADD + ELU): bytes it must move to and from HBM, operations the matrix unit performs (the padded tiles), the two
    times in us"""
    es = 2 if dtype_name == "float16" else 4
    pad = lambda n: -(-n // 32) * 32          # noqa: E731
    Cout, bands = max(Ci, Co), -(-HP // ROWS)
    x, act, w = M * HP * 12 * Ci * es, M * HP * 12 * Cout * es, 9 * Ci * Co
    packed = 9 * pad(Ci) * pad(Co) * es
    part = -(-M // W_SAMPLES) * (w + Co) * 4
    conv_ops = 2 * M * bands * ROWS * 12 * 9 * pad(Ci) * pad(Co)
    rows = {"k_res_pack": (w * es + packed, 0),
            "k_res_conv_fwd": (x + act + packed, conv_ops),
            "k_res_conv_grad_x": (2 * act + x + packed, conv_ops),
            "k_res_grad_w": (x + 2 * act + part, 2 * M * bands * ROWS * 16 * 9 * pad(Ci) * Co),
            "k_res_grad_w_reduce": (part + w * 4, 0)}
    res = {}
    for name, (nbytes, ops) in rows.items():
        t_mem, t_mat = nbytes / HBM * 1e6, ops / PEAK[dtype_name] * 1e6
        res[name] = {"bytes": nbytes, "operations": ops, "us_at_8_TB_per_s": round(t_mem, 2), "us_at_matrix_peak": round(t_mat, 2),
                     "bound": "memory" if t_mem >= t_mat else "matrix", "us_bound": round(max(t_mem, t_mat), 2)}
    return res


def time_paths(torch, paths):
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


def make_paths(torch, ti, te, M, dtype, layout, channels):
    """channels: (Ci, Co, Co, ...) — one layer, or a block of several"""
    gen = torch.Generator(device="cuda").manual_seed(M)
    rand = lambda *s: 2 * torch.rand(*s, device="cuda", generator=gen) - 1            # noqa: E731
    x = rand(M, HP, 12, channels[0]).to(dtype).permute(0, 3, 1, 2)                    # [M, Ci, Hp, 12] over NHWC memory
    if layout == "channels_first":
        x = x.contiguous()
    x.requires_grad_()
    params, Cin = [], channels[0]
    for Co in channels[1:]:
        params.append(((rand(3, 3, Cin, Co) * (6.0 / (9 * Cin + 9 * Co)) ** 0.5).requires_grad_(), (rand(Co) / 16).requires_grad_()))   # float32 masters
        Cin = max(Cin, Co)
    G = rand(M, HP, 12, Cin).to(dtype).permute(0, 3, 1, 2)
    leaves = [x] + [t for p in params for t in p]

    def lib():
        return te.residual_block(x, params)

    def composed():
        y = x
        for w, bias in params:
            y = ref_residual_layer(y, w.to(dtype), bias.to(dtype), "add", "elu").permute(0, 3, 1, 2)
        return y

    def no_grad(fn):
        def run():
            with torch.no_grad():
                return fn()
        return run

    return {"fwd": no_grad(lib), "fwd_bwd": lambda: torch.autograd.grad(lib(), leaves, G),
            "torch_fwd": no_grad(composed), "torch_fwd_bwd": lambda: torch.autograd.grad(composed(), leaves, G)}


def same(torch, got, want, dtype, what):
    tol = 2e-2 if dtype == torch.float16 else 1e-4
    for g, t in zip(got, want):
        top = max(float(t.float().abs().max()), 1e-3)
        assert float((g.float() - t.float().reshape(g.shape)).abs().max()) <= tol * top, f"{what}: the two paths differ"


def versus(us, new, old):
    n_, o_ = us[new], us[old]
    return {"new": new, "old": old, "faster_in_every_window": all(a < b for a, b in zip(n_["windows"], o_["windows"])),
            "spreads_do_not_overlap": n_["max"] < o_["min"], "old_over_new": round(o_["median"] / n_["median"], 2)}


def main():
    import torch
    arg = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default          # noqa: E731
    dst = arg("--out", os.path.join(ROOT, "profiles", "res"))
    path = os.path.join(dst, "res_layer.json")
    if "--stats" in sys.argv:
        return merge_stats(path, arg("--stats", None))
    if "--kernels" in sys.argv:
        return kernels_only(torch)
    sizes = [int(v) for v in arg("--sizes", "1024,4096,16384").split(",")]
    ti = importlib.import_module("drl-tetris_amd.torch_interop")
    pkg = ge.package()
    out = {"note": __doc__, "calls_per_window": CALLS, "shape": {"Hp": HP, "Ci": CH, "Co": CH, "join": "add", "activation": "elu"}, "cases": {}}

    def save():
        os.makedirs(dst, exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
    b = pkg.TetrisBatch(8, 1, 20, 10, device=0)
    te = ti.TorchEnv(b)
    mid = sizes[len(sizes) // 2]
    cases = [(M, dn, layout, (CH, CH)) for layout in ("channels_last", "channels_first") for M in sizes for dn in ("float32", "float16")]
    cases += [(mid, dn, "channels_last", (136, CH)) for dn in ("float32", "float16")]
    cases += [(mid, dn, "channels_last", (CH, CH, CH, CH)) for dn in ("float32", "float16")]
    for M, dn, layout, channels in cases:          # a case at a time: compared, warmed, timed; its tensors are dropped before the next
        dtype = getattr(torch, dn)
        paths = make_paths(torch, ti, te, M, dtype, layout, channels)
        same(torch, [paths["fwd"]().clone()], [paths["torch_fwd"]()], dtype, "forward")
        same(torch, [t.clone() for t in paths["fwd_bwd"]()], paths["torch_fwd_bwd"](), dtype, "backward")
        for fn in paths.values():
            for _ in range(WARMUP):
                fn()
        r = {"clock_mhz": [b.clock_mhz()]}
        us = r["us_per_call"] = time_paths(torch, paths)
        r["clock_mhz"].append(b.clock_mhz())
        r["versus_torch"] = [versus(us, n, "torch_" + n) for n in ("fwd", "fwd_bwd")]
        if len(channels) == 2:
            bd = bounds(M, dn, channels[0], channels[1])
            r["bound_us"] = {"fwd": bd["k_res_conv_fwd"]["us_bound"], "fwd_bwd": round(sum(v["us_bound"] for kname, v in bd.items() if kname != "k_res_pack"), 2)}
        name = f"{M}_{dn}_{layout}" + ("" if channels == (CH, CH) else "_block3" if len(channels) > 2 else f"_Ci{channels[0]}")
        out["cases"][name] = r
        print(name, json.dumps({k: v["median"] for k, v in us.items()}), json.dumps(r["versus_torch"]), flush=True)
        save()
        del paths
        te._loss_cache = None
        torch.cuda.empty_cache()
    out["errors"] = b.take_errors()
    b.set_stream(None, external=False)
    b.close()
    save()


def kernels_only(torch, M=16384, reps=10):
    pkg = ge.package()
    b = pkg.TetrisBatch(8, 1, 20, 10, device=0)
    b.set_stream(torch.cuda.current_stream().cuda_stream, external=True)
    p = lambda t: C.c_void_p(t.data_ptr())                                   # noqa: E731
    for dtype in (torch.float32, torch.float16):
        rand = lambda *s: (2 * torch.rand(*s, device="cuda") - 1)             # noqa: E731
        x, w, g = rand(M, HP, 12, CH).to(dtype), (rand(3, 3, CH, CH) / 16).to(dtype), rand(M, HP, 12, CH).to(dtype)
        bias, out, gx = rand(CH), torch.zeros_like(x), torch.zeros_like(x)
        gw, gb = torch.zeros(3, 3, CH, CH, device="cuda"), torch.zeros(CH, device="cuda")
        r = b.res_layer(M, HP, CH, CH, x=p(x), w=p(w), bias=p(bias), y=p(out), grad_out=p(g), out=p(out), grad_x=p(gx), grad_w=p(gw), grad_b=p(gb),
                        f16=dtype == torch.float16)
        for _ in range(reps):
            b.res_layer_dev(r)
            b.res_layer_grad_x_dev(r)
            b.res_layer_grad_w_dev(r)
        torch.cuda.synchronize()
    b.set_stream(None, external=False)
    b.close()


def merge_stats(path, stats_csv, M=16384):
    with open(path) as f:
        out = json.load(f)
    rows = list(csv.DictReader(open(stats_csv)))
    res = {}
    for row in rows:
        name = row.get("Name") or row.get("KernelName") or ""
        found = re.search(r"k_res_(pack|conv|grad_w_reduce|grad_w)", name)
        if not found:
            continue
        flags = re.findall(r"Lb([01])E", name) or [("1" if t == "true" else "0") for t in re.findall(r"true|false", name)]
        dn = "float16" if flags and flags[0] == "1" else "float32"
        short = found.group(0)
        if short == "k_res_conv":
            short += "_fwd" if flags[1] == "1" else "_grad_x"
        bd = bounds(M, dn).get(short)
        avg = float(row.get("AverageNs") or row.get("Average") or 0.0) / 1000.0
        entry = {"kernel": name, "calls": int(float(row.get("Calls") or 0)), "us_average": round(avg, 2), "us_min": round(float(row.get("MinNs") or 0) / 1000.0, 2),
                 "us_max": round(float(row.get("MaxNs") or 0) / 1000.0, 2)}
        if bd:
            entry["type"] = dn if short != "k_res_grad_w_reduce" else "float32 partials (both types' calls)"
            entry.update(bd)
            entry["bound_over_time"] = round(bd["us_bound"] / avg, 3) if avg else None
        res.setdefault(short, []).append(entry)
    out["kernels"] = {"M": M, "note": "rocprofv3 --kernel-trace --stats, a run of its own; k_res_grad_w_reduce has no element type: its calls of both types are one row",
                      "rows": res}
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
