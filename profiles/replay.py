"""Cost of the prioritised experience replay on the device: the library calls (tetris_replay_add_dev, tetris_replay_sample_dev,
tetris_replay_gather_dev, tetris_replay_update_prios_dev through TorchEnv.replay) and, for the sample, the same draw composed from
torch ops.

    python profiles/replay.py [--out DIR] [--sizes 65536,524288,2097152]    -> DIR/replay.json (default profiles/replay)

Two-player 20x10 games.  Paths:
  add_<N>                Replay.add of a window of 32 rows of N = 4 096 and 65 536 games, `closed` with a done on one row in 40,
                         augment; the ring holds 2^22 entries, so the cursor wraps every few calls
  sample_<size>_<M>      Replay.sample(M, 0.7, 0.5) on a full ring of max_size = size random priorities, M = 256 and 16 384
  torch_sample_<size>_<M>  a stable argsort of the priorities, the scatter of the ranks, pow, rand, log, divide, topk(M, smallest)
                         and the weights' pow: what a user composes without the library (its uniforms are torch's own, so only
                         the ranks are compared before anything is timed)
  gather_<size>_<M>      Replay.gather(index, steps=6) of the sample's M indices (k_step = 5)
  update_<size>_<M>      Replay.update_prios(index, weight)
A window = HIP events around 20 calls, nothing synchronised inside; five windows per path, the paths taken in turn within every
repeat, after a warm-up of every path.  The shader clock (tetris_debug_clock_khz) is read before and after each case.  Reported per
path: the windows, their median, lowest and highest (us per call)."""
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
H, P, K_STEP = 20, 2, 5
ADD_ROWS, ADD_GAMES, ADD_RING = 32, (4096, 65536), 1 << 22
SAMPLE_M = (256, 16384)
ALPHA, BETA = 0.7, 0.5


def measure(paths, b):
    import torch
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
    out["errors"] = b.take_errors()
    return out


def batch_of(n):
    ti = importlib.import_module("drl-tetris_amd.torch_interop")
    b = ge.package().TetrisBatch(n, P, H, 10, seeds=orc.episode_seed(np.arange(n), 0), device=0)
    return b, ti.TorchEnv(b)


def close(b):
    b.set_stream(None, external=False)
    b.close()


def add_case(n):
    import torch
    b, te = batch_of(n)
    b.rollout_random(1, 20)
    gen = torch.Generator(device="cuda").manual_seed(0)
    tr = te.trajectory(ADD_ROWS, states=True)
    player = (torch.arange(n, device="cuda") % P).to(torch.uint8)
    for row in range(ADD_ROWS):
        tr.observe(row, player)
    tr.action.copy_(torch.stack([torch.randint(0, hi, (ADD_ROWS, n), generator=gen, device="cuda") for hi in (4, 10, 7, 2)], dim=2).to(torch.uint8))
    for x in (tr.prob, tr.reward, tr.adv, tr.target):
        x.copy_(torch.randn(ADD_ROWS, n, generator=gen, device="cuda"))
    tr.done.copy_((torch.rand(ADD_ROWS, n, generator=gen, device="cuda") < 1.0 / 40.0).to(torch.uint8))
    tr.closed.copy_(tr.done.flip(0).cummax(0).values.flip(0))
    tr._rows = ADD_ROWS
    rp = te.replay(ADD_RING + K_STEP, k_step=K_STEP)
    rp.add(tr, ADD_ROWS)
    k = 2 * int(tr.closed.sum().item())
    assert len(rp) == k and rp.dropped() == 0
    out = measure({f"add_{n}": lambda: rp.add(tr, ADD_ROWS)}, b)
    out["entries_per_call"] = k
    out["bytes_per_call"] = k * (48 * P + 4 + 16 + 2 + 4) * 2
    assert rp.dropped() == 0
    close(b)
    return out


def sample_case(size):
    import torch
    b, te = batch_of(64)
    gen = torch.Generator(device="cuda").manual_seed(1)
    rp = te.replay(size + K_STEP, k_step=K_STEP, seed=3)
    rp.prio.copy_(torch.rand(size, generator=gen, device="cuda"))
    rp.prio[: size // 4] = 2.0                            # a block of entries fresh from an add
    rp.obs.copy_(torch.randint(0, 1 << 20, tuple(rp.obs.shape), generator=gen, device="cuda", dtype=torch.int32))
    rp.cursor.copy_(torch.tensor([0, size, size, 0], dtype=torch.int32))
    n_f = float(size)

    def torch_sample(M):
        order = torch.argsort(rp.prio, stable=True)
        rank = torch.empty(size, dtype=torch.int64, device="cuda")
        rank[order] = size - torch.arange(size, device="cuda")
        w = rank.to(torch.float32).pow(-ALPHA)
        key = -torch.log(1.0 - torch.rand(size, device="cuda")) / w
        idx = torch.topk(key, M, largest=False, sorted=True).indices
        return idx.to(torch.int32), (rank[idx].to(torch.float32) / n_f).pow(ALPHA * BETA), rank

    rp.sample(256, ALPHA, BETA, draw=0, rank=True)
    assert torch.equal(rp.rank.to(torch.int64), torch_sample(256)[2]), "ranks of the torch composition"
    paths, index = {}, {}
    draw = {"k": 0}

    def sample(M):
        draw["k"] += 1
        return rp.sample(M, ALPHA, BETA, draw=draw["k"])

    for M in SAMPLE_M:
        idx, weight, count = sample(M)
        assert int(count.item()) == M
        index[M] = (idx.clone(), weight.clone())
        paths[f"sample_{size}_{M}"] = lambda M=M: sample(M)
        paths[f"torch_sample_{size}_{M}"] = lambda M=M: torch_sample(M)
        paths[f"gather_{size}_{M}"] = lambda M=M: rp.gather(index[M][0], steps=K_STEP + 1)
        paths[f"update_{size}_{M}"] = lambda M=M: rp.update_prios(*index[M])
    out = measure(paths, b)
    us = out["us_per_call"]
    out["comparison"] = []
    for M in SAMPLE_M:
        a, o = us[f"sample_{size}_{M}"], us[f"torch_sample_{size}_{M}"]
        out["comparison"].append({"new": f"sample_{size}_{M}", "old": f"torch_sample_{size}_{M}",
                                  "faster_in_every_window": all(x < y for x, y in zip(a["windows"], o["windows"])),
                                  "spreads_do_not_overlap": a["max"] < o["min"], "old_over_new": round(o["median"] / a["median"], 2)})
    out["sort_scratch_bytes"] = 20 * size + 4 * 256 * ((size + 2047) // 2048) + 1024
    close(b)
    return out


def main():
    dst = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "replay")
    sizes = [int(v) for v in sys.argv[sys.argv.index("--sizes") + 1].split(",")] if "--sizes" in sys.argv else [65536, 524288, 2097152]
    out = {"note": __doc__, "calls_per_window": CALLS, "cases": {}}
    os.makedirs(dst, exist_ok=True)
    for name, fn, arg in [(f"add_{n}", add_case, n) for n in ADD_GAMES] + [(f"sample_{s}", sample_case, s) for s in sizes]:
        r = fn(arg)
        out["cases"][name] = r
        print(name, json.dumps({k: v["median"] for k, v in r["us_per_call"].items()}), json.dumps(r.get("comparison", "")), flush=True)
        with open(os.path.join(dst, "replay.json"), "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
