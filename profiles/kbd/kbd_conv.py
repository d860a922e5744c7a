"""Cost of the keyboard convolution: TorchEnv.keyboard_conv (tetris_kbd_conv_dev and its _grad_x_dev / _grad_w_dev) against the same
layer composed from torch ops on the same tensors — F.conv2d on the input, the four slices, cat (tests/kbd_support.py:
ref_keyboard_conv) —, forward under no_grad and forward plus torch.autograd.grad with a dense incoming gradient.

    python profiles/kbd/kbd_conv.py [--out DIR] [--sizes 1024,4096,16384] [--variant NAME=LIB ...]   -> DIR/kbd_conv.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o kbd -- python profiles/kbd/kbd_conv.py --kernels     (a run of its own)
    python profiles/kbd/kbd_conv.py --out DIR --stats DIR/kbd_kernel_stats.csv      -> adds "kernels" to the json

Hp = 22, C = 128, K = 7, float32 and float16, M = 1 024, 4 096 and 16 384, once with a channels_last input and once with a
channels-first one on both sides, so that the layout copy is counted where it occurs (the library's wrapper copies; torch's
conv2d chooses for itself).  A window = HIP events around 20 calls, nothing synchronised inside; five windows per path, the paths
of a case taken in turn within every repeat, after a warm-up of every path of every case (torch's convolution picks its algorithm
on first use).  The clock is noted before and after a case.  The outputs of both sides are compared before anything is timed.
--variant times the library paths of another build of the library (another KBD_BLOCK: hipcc -DTETRIS_KBD_BLOCK=8 or 32) at the
largest size, in the same process, taken in turn with the committed one.
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
from tests.kbd_support import ref_keyboard_conv  # noqa: E402

CALLS, WINDOWS, WARMUP = 20, 5, 3
HBM, PEAK = 8.0e12, {"float16": 2516.8e12, "float32": 157.3e12}
HP, CH, K = 22, 128, 7
O, OP = 4 * K, 32


def bounds(M, dtype_name):
    """per kernel: bytes it must move to and from HBM, operations the matrix unit performs (the padded tiles), the two times in us"""
    es = 2 if dtype_name == "float16" else 4
    x, w, out = M * HP * 12 * CH * es, HP * 3 * CH * O, M * 40 * K * es
    packed = HP * 3 * OP * CH * es
    chunks = -(-M // 256)
    part = chunks * (HP * 3 * CH * OP + OP) * 4
    rows = {"k_kbd_pack": (w * es + packed, 0),
            "k_kbd_fwd": (x + out + packed, 2 * M * 10 * OP * HP * 3 * CH),
            "k_kbd_grad_x": (x + out + packed, 2 * M * 12 * 96 * HP * CH),
            "k_kbd_grad_w": (x + out * HP + part, 2 * -(-M // 8) * 96 * 96 * HP * CH),
            "k_kbd_grad_w_reduce": (part + w * 4, 0)}
    res = {}
    for name, (nbytes, ops) in rows.items():
        t_mem, t_mat = nbytes / HBM * 1e6, ops / PEAK[dtype_name] * 1e6
        res[name] = {"bytes": nbytes, "operations": ops, "us_at_8_TB_per_s": round(t_mem, 2), "us_at_matrix_peak": round(t_mat, 2),
                     "bound": "memory" if t_mem >= t_mat else "matrix", "us_bound": round(max(t_mem, t_mat), 2)}
    return res


def time_paths(torch, paths, warm=True):
    if warm:
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


def make_paths(torch, te, M, dtype, layout, prefix="", with_torch=True):
    gen = torch.Generator(device="cuda").manual_seed(M)
    rand = lambda *s: 2 * torch.rand(*s, device="cuda", generator=gen) - 1            # noqa: E731
    x = rand(M, HP, 12, CH).to(dtype).permute(0, 3, 1, 2)                     # [M, C, Hp, 12] over NHWC memory
    if layout == "channels_first":
        x = x.contiguous()
    x.requires_grad_()
    w = (rand(HP, 3, CH, O) / 16).requires_grad_()                           # the float32 master weight
    bias = (rand(O) / 16).requires_grad_()
    G = rand(M, 4, 10, K).to(dtype)

    def lib():
        return te.keyboard_conv(x, w, bias)

    def composed():
        return ref_keyboard_conv(x, w.to(dtype), bias.to(dtype), 4, K)

    def no_grad(fn):
        def run():
            with torch.no_grad():
                return fn()
        return run

    paths = {prefix + "fwd": no_grad(lib), prefix + "fwd_bwd": lambda: torch.autograd.grad(lib(), (x, w, bias), G)}
    if with_torch:
        paths.update({"torch_fwd": no_grad(composed), "torch_fwd_bwd": lambda: torch.autograd.grad(composed(), (x, w, bias), G)})
    return paths


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
    dst = arg("--out", os.path.join(ROOT, "profiles", "kbd"))
    path = os.path.join(dst, "kbd_conv.json")
    if "--stats" in sys.argv:
        return merge_stats(path, arg("--stats", None))
    if "--kernels" in sys.argv:
        return kernels_only(torch)
    sizes = [int(v) for v in arg("--sizes", "1024,4096,16384").split(",")]
    libs = [tuple(sys.argv[i + 1].split("=", 1)) for i, t in enumerate(sys.argv) if t == "--variant"]
    ti = importlib.import_module("drl-tetris_amd.torch_interop")
    pkg = ge.package()
    out = {"note": __doc__, "calls_per_window": CALLS, "shape": {"Hp": HP, "C": CH, "K": K}, "cases": {}}

    def save():
        os.makedirs(dst, exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
    b = pkg.TetrisBatch(8, 1, 20, 10, device=0)
    te = ti.TorchEnv(b)
    cases = [(M, dn, layout) for layout in ("channels_last", "channels_first") for M in sizes for dn in ("float32", "float16")]
    made = {}
    for M, dn, layout in cases:                 # every shape first: compared, and warm
        dtype = getattr(torch, dn)
        paths = made[(M, dn, layout)] = make_paths(torch, te, M, dtype, layout)
        same(torch, [paths["fwd"]().clone()], [paths["torch_fwd"]()], dtype, "forward")
        same(torch, [t.clone() for t in paths["fwd_bwd"]()], paths["torch_fwd_bwd"](), dtype, "backward")
        for fn in paths.values():
            for _ in range(WARMUP):
                fn()
    for M, dn, layout in cases:
        r = {"clock_mhz": [b.clock_mhz()]}
        us = r["us_per_call"] = time_paths(torch, made[(M, dn, layout)], warm=False)
        r["clock_mhz"].append(b.clock_mhz())
        r["versus_torch"] = [versus(us, n, "torch_" + n) for n in ("fwd", "fwd_bwd")]
        bd = bounds(M, dn)
        r["bound_us"] = {"fwd": bd["k_kbd_fwd"]["us_bound"], "fwd_bwd": round(sum(v["us_bound"] for kname, v in bd.items() if kname != "k_kbd_pack"), 2)}
        out["cases"][f"{M}_{dn}_{layout}"] = r
        print(M, dn, layout, json.dumps({k: v["median"] for k, v in us.items()}), json.dumps(r["versus_torch"]), flush=True)
        save()
        del made[(M, dn, layout)]
    out["errors"] = b.take_errors()
    if libs:
        out["block_variants"] = {}
        for dn in ("float16", "float32"):
            paths, batches = make_paths(torch, te, sizes[-1], getattr(torch, dn), "channels_last", prefix="block16_", with_torch=False), []
            for name, lib in libs:
                vb = pkg.TetrisBatch(8, 1, 20, 10, device=0, lib_path=lib)
                batches.append(vb)
                paths.update(make_paths(torch, ti.TorchEnv(vb), sizes[-1], getattr(torch, dn), "channels_last", prefix=name + "_", with_torch=False))
            us = out["block_variants"][f"{sizes[-1]}_{dn}"] = time_paths(torch, paths)
            print("variants", dn, json.dumps({k: v["median"] for k, v in us.items()}), flush=True)
            for vb in batches:
                vb.set_stream(None, external=False)
                vb.close()
            save()
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
        x, w, g = rand(M, HP, 12, CH).to(dtype), (rand(HP, 3, CH, O) / 16).to(dtype), rand(M, 4, 10, K).to(dtype)
        bias, out, gx = rand(O), torch.zeros(M, 4, 10, K, device="cuda", dtype=dtype), torch.zeros_like(x)
        gw, gb = torch.zeros(HP, 3, CH, O, device="cuda"), torch.zeros(O, device="cuda")
        k = b.kbd_conv(M, HP, CH, K, x=p(x), w=p(w), bias=p(bias), grad_out=p(g), out=p(out), grad_x=p(gx), grad_w=p(gw), grad_b=p(gb),
                       f16=dtype == torch.float16)
        for _ in range(reps):
            b.kbd_conv_dev(k)
            b.kbd_conv_grad_x_dev(k)
            b.kbd_conv_grad_w_dev(k)
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
        found = re.search(r"k_kbd_(pack|fwd|grad_x|grad_w_reduce|grad_w)", name)
        if not found:
            continue
        dn = "float16" if "ILb1E" in name or "<true" in name else "float32"          # (mangled or demangled)
        short = found.group(0)
        bd = bounds(M, dn).get(short)
        avg = float(row.get("AverageNs") or row.get("Average") or 0.0) / 1000.0
        entry = {"kernel": name, "calls": int(float(row.get("Calls") or 0)), "us_average": round(avg, 2), "us_min": round(float(row.get("MinNs") or 0) / 1000.0, 2),
                 "us_max": round(float(row.get("MaxNs") or 0) / 1000.0, 2)}
        if bd:
            entry["type"] = dn if short != "k_kbd_grad_w_reduce" else "float32 partials (both types' calls)"
            entry.update(bd)
            entry["bound_over_time"] = round(bd["us_bound"] / avg, 3) if avg else None
        res.setdefault(short, []).append(entry)
    out["kernels"] = {"M": M, "note": "rocprofv3 --kernel-trace --stats, a run of its own; k_kbd_grad_w_reduce has no element type: its calls of both types are one row",
                      "rows": res}
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
