"""Cost of the network's input side: Trajectory.inputs (tetris_net_input_dev: one launch from the packed records) against the same
result composed from torch ops on Trajectory.batch's uint8 planes — the cast, the two pads, cumsum, minimum, the subtraction, the
height plane, cat and, for channels-last, .contiguous(memory_format=torch.channels_last).

    python profiles/input/net_input.py [--out DIR] [--sizes 4096,16384,65536] [--variant NAME=LIB ...]  -> DIR/net_input.json

M = 4 096, 16 384 and 65 536 samples of a window of two-player games at H = 20 (an index list of distinct entries, half of them
mirrored), C = 1 (no item), 4 (cumsum, shadow, height: the reference's `items=True`) and 5 (all four), channels-first and
channels-last, float32 and float16, with the pad, torch's stream.  Paths per case:
  torch_inputs   tr.batch(index) — its launch counts on this side — and the composition above on its visual and vector
  inputs         tr.inputs(index, ...): the library, one launch; batch is not called
A window = HIP events around 20 calls, nothing synchronised inside; five windows per path, the paths taken in turn within every
repeat, after a warm-up of each.  `bytes` is what the library's call writes — S M (C Hp Wp + 12) elements, S M + M bytes of piece
and valid — `TB_per_s` is it over the median; the 48 S M bytes it reads are under 2 % of that.  The outputs of both sides are compared
before anything is timed.  --variant times tr.inputs of another build of the library (another kernel form, other samples per
workgroup) at the largest size, in the same process, taken in turn with the committed one."""
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import __graft_entry__ as ge  # noqa: E402

CALLS, WINDOWS, WARMUP = 20, 5, 3
PEAK = 8.0e12
H, S = 20, 2
ITEM_SETS = {1: (), 4: ("cumsum", "shadow", "height"), 5: ("cumsum", "shadow", "height", "holes")}


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


def make_window(torch, lib=None):
    """a window of 4 rows of 16 384 two-player games whose records are random boards (rows 0..H-1 of every column) with well-formed
    scalar words -> (batch, TorchEnv, Trajectory)"""
    ti = importlib.import_module("drl-tetris_amd.torch_interop")
    pkg = ge.package()
    n, rows = 16384, 4
    b = pkg.TetrisBatch(n, S, H, 10, device=0, **({"lib_path": lib} if lib else {}))
    te = ti.TorchEnv(b)
    tr = te.trajectory(rows, states=True)
    gen = torch.Generator(device="cuda").manual_seed(11)
    bits = lambda hi, *shape: torch.randint(0, hi, shape, device="cuda", generator=gen, dtype=torch.int64)            # noqa: E731
    cols = bits(1 << H, rows, n, S, 10) & bits(1 << H, rows, n, S, 10)              # about a quarter of the cells
    w10 = bits(1 << 31, rows, n, S, 1)
    w11 = bits(256, rows, n, S, 1) | (bits(8, rows, n, S, 1) << 8) | (bits(8, rows, n, S, 1) << 16)
    tr.obs.copy_(torch.cat([cols, w10, w11], dim=3).to(torch.int32))
    return b, te, tr


def torch_inputs(torch, tr, index, items, dtype, channels_last):
    F = torch.nn.functional
    mb = tr.batch(index)
    x = mb.visual.to(dtype)                                                          # [S, M, H, 10]
    x = F.pad(x, (0, 0, 1, 0), value=0.0)                                            # a zero row on top
    x = F.pad(x, (1, 1, 0, 1), value=1.0)                                            # ones left, right and below
    x = x.unsqueeze(2)                                                               # [S, M, 1, Hp, Wp]
    planes = [x]
    if items:
        cumsum = torch.cumsum(x, dim=3)
        shadow = torch.minimum(cumsum, torch.ones((), dtype=dtype, device=x.device))
        by_name = {"cumsum": cumsum, "shadow": shadow}
        if "height" in items:
            by_name["height"] = torch.arange(x.shape[3], dtype=dtype, device=x.device).reshape(1, 1, 1, -1, 1).expand_as(x)
        if "holes" in items:
            by_name["holes"] = shadow - x
        planes += [by_name[i] for i in items]
    out = torch.cat(planes, dim=2) if len(planes) > 1 else x
    if channels_last:
        out = out.flatten(0, 1).contiguous(memory_format=torch.channels_last).unflatten(0, x.shape[:2])
    return out, mb.vector.to(dtype), mb.piece, mb.valid


def case(torch, tr, b, M, C, dtype_name, channels_last):
    dtype = getattr(torch, dtype_name)
    items = ITEM_SETS[C]
    gen = torch.Generator(device="cuda").manual_seed(M + C)
    total = tr.capacity * b.n_games
    index = torch.randperm(total, device="cuda", generator=gen)[:M].to(torch.int32)
    index[::2] |= -(1 << 31)                                                         # every other sample mirrored
    index = index.contiguous()
    paths = {"torch_inputs": lambda: torch_inputs(torch, tr, index, items, dtype, channels_last),
             "inputs": lambda: tr.inputs(index, items=items, pad=True, dtype=dtype, channels_last=channels_last)}
    got, want = paths["inputs"](), paths["torch_inputs"]()
    torch.cuda.synchronize()
    for g, w, name in zip(got, want, ("visual", "vector", "piece", "valid")):
        assert g.shape == w.shape and torch.equal(g, w), f"{name}: the two paths differ"
    if channels_last and C > 1:
        assert got[0].stride() == want[0].stride(), "the same memory layout"
    out = {"clock_mhz": [b.clock_mhz()]}
    us = out["us_per_call"] = time_paths(torch, paths)
    out["clock_mhz"].append(b.clock_mhz())
    esize = 2 if dtype == torch.float16 else 4
    nbytes = S * M * (C * (H + 2) * 12 + 12) * esize + S * M + M
    med = us["inputs"]["median"]
    out["bandwidth"] = {"bytes_written": nbytes, "us": med, "TB_per_s": round(nbytes / med / 1e6, 3),
                        "share_of_8_TB_per_s": round(nbytes / med / 1e6 / (PEAK / 1e12), 3)}
    n_, o_ = us["inputs"], us["torch_inputs"]
    out["versus_torch"] = {"faster_in_every_window": all(x < y for x, y in zip(n_["windows"], o_["windows"])),
                           "spreads_do_not_overlap": n_["max"] < o_["min"], "old_over_new": round(o_["median"] / n_["median"], 2)}
    return out


def variants(torch, tr, M, libs):
    """tr.inputs of the committed build and of other builds on the same records, every layout and type at C = 5, taken in turn"""
    others = []
    for name, lib in libs:
        b2, te2, tr2 = make_window(torch, lib)
        tr2.obs.copy_(tr.obs)
        others.append((name, b2, tr2))
    gen = torch.Generator(device="cuda").manual_seed(M)
    index = torch.randperm(tr.capacity * tr.env.b.n_games, device="cuda", generator=gen)[:M].to(torch.int32).contiguous()
    out = {}
    for dtype_name in ("float32", "float16"):
        for cl in (False, True):
            kw = dict(items=ITEM_SETS[5], pad=True, dtype=getattr(torch, dtype_name), channels_last=cl)
            paths = {"committed": lambda kw=kw: tr.inputs(index, **kw)}
            for name, _, tr2 in others:
                paths[name] = lambda kw=kw, tr2=tr2: tr2.inputs(index, **kw)
                a, c = tr.inputs(index, **kw)[0], tr2.inputs(index, **kw)[0]
                torch.cuda.synchronize()
                assert torch.equal(a, c), f"{name}: the variant's output differs"
            out[f"{M}_C5_{dtype_name}_{'last' if cl else 'first'}"] = time_paths(torch, paths)
    for _, b2, _ in others:
        b2.set_stream(None, external=False)
        b2.close()
    return out


def main():
    import torch
    arg = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default          # noqa: E731
    dst = arg("--out", os.path.join(ROOT, "profiles", "input"))
    sizes = [int(x) for x in arg("--sizes", "4096,16384,65536").split(",")]
    libs = [tuple(sys.argv[i + 1].split("=", 1)) for i, t in enumerate(sys.argv) if t == "--variant"]
    out = {"note": __doc__, "calls_per_window": CALLS, "cases": {}}

    def save():
        os.makedirs(dst, exist_ok=True)
        with open(os.path.join(dst, "net_input.json"), "w") as f:
            json.dump(out, f, indent=1)
    b, te, tr = make_window(torch)
    for M in sizes:
        for C in (1, 4, 5):
            for dtype_name in ("float32", "float16"):
                for cl in (False, True):
                    r = case(torch, tr, b, M, C, dtype_name, cl)
                    out["cases"][f"{M}_C{C}_{dtype_name}_{'last' if cl else 'first'}"] = r
                    print(M, C, dtype_name, "last" if cl else "first", json.dumps({k: x["median"] for k, x in r["us_per_call"].items()}),
                          json.dumps(r["versus_torch"]), r["bandwidth"]["TB_per_s"], flush=True)
                    save()
    slower = [k for k, r in out["cases"].items() if not r["versus_torch"]["faster_in_every_window"]]
    out["not_faster_in_every_window"] = slower
    largest = out["cases"][f"{sizes[-1]}_C5_float32_first"]["bandwidth"]
    out["largest_case"] = dict(largest, case=f"{sizes[-1]}_C5_float32_first")
    save()
    if libs:
        out["variants"] = variants(torch, tr, sizes[-1], libs)
        for k, us in out["variants"].items():
            print("variants", k, json.dumps({name: x["median"] for name, x in us.items()}), flush=True)
        save()
    out["errors"] = b.take_errors()
    save()
    b.set_stream(None, external=False)
    b.close()


if __name__ == "__main__":
    main()
