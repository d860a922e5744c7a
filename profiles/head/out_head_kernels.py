"""The four output-head kernels alone, for a kernel trace: ten calls of each entry point through capi (no autograd, no wrapper) at
M = 65 536, K = 7, Kv = 7, W = 8, float32 and float16, the Q head in mode MEAN with the mask {0, 2, 5}.

    rocprofv3 --kernel-trace --stats -d DIR -o head -- python profiles/head/out_head_kernels.py

The kernels' own times are in DIR's kernel statistics; out_head.py's windows hold the wrappers' host time as well."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import __graft_entry__ as ge  # noqa: E402

M, K, REPS = 65536, 7, 10


def main():
    import torch
    pkg = ge.package()
    b = pkg.TetrisBatch(8, 1, 20, 10, device=0)
    b.set_stream(torch.cuda.current_stream().cuda_stream, external=True)
    p = lambda t: C.c_void_p(t.data_ptr())                                   # noqa: E731
    for dtype in (torch.float32, torch.float16):
        big = lambda: (2 * torch.rand(M, 4, 10, K, device="cuda") - 1).to(dtype)          # noqa: E731
        small = lambda n: (2 * torch.rand(M, n, device="cuda") - 1).to(dtype)             # noqa: E731
        a, v, G, Q, A, ga, gv = big(), small(K), big(), big(), big(), big(), small(K)
        V = torch.zeros(M, device="cuda")
        f16 = dtype == torch.float16
        q = b.q_head(p(a), M, v=p(v), n_pieces=K, n_values=K, mode="mean", advantage_range=0.5, used_pieces=0b0100101, f16=f16, value_f16=f16,
                     Q=p(Q), V=p(V), grad_Q=p(G), grad_a=p(ga), grad_v=p(gv))
        x, w, pi, pv, g, gpv, gx, gw = big(), small(K + 1), big(), small(K), big(), small(K), big(), small(K + 1)
        ph = b.policy_head(M, p(pi), p(pv), n_pieces=K, n_values=K + 1, x=p(x), w=p(w), grad_pi=p(g), grad_v=p(gpv), grad_x=p(gx), grad_w=p(gw),
                           f16=f16, value_f16=f16)
        for _ in range(REPS):
            b.q_head_dev(q)
            b.q_head_grad_dev(q)
            b.policy_head_dev(ph)
            b.policy_head_grad_dev(ph)
        torch.cuda.synchronize()
    b.set_stream(None, external=False)
    b.close()


if __name__ == "__main__":
    main()
