"""Time the static-grid PDE primitive (sigsvgd_pde_fwd_bwd) at the notebook shape next to the coverage kernel.

    python scripts/pde_time.py [--N 100 --T 10 --d 2 --order 4 --reps 50]

Prints one JSON line: milliseconds per launch (median of `reps` timed with device events after warm-up) of
  pde_fwd, pde_fwd_bwd      on the [N*N, T, T] RBF grid (the grid itself is built once, outside the timing);
  generic_ordered / _sym    gram_fwd_bwd(force_generic=True) -- the coverage kernel, every ordered pair / each unordered
                            pair once (Y_IS_X);
  user_gram_and_grad        SigKernel(<RBF behind Gram_matrix only>).gram_and_grad(X): grid, PDE and chain rule.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from sigsvgd_amd import ops  # noqa: E402
import sigsvgd_amd.sigkernel as sk  # noqa: E402
from sigsvgd_amd.utils.synthetic import synthetic_inputs  # noqa: E402


class _GramOnlyRBF:
    def __init__(self, sigma):
        self.sigma = sigma

    def Gram_matrix(self, X, Y):
        return sk.RBFKernel(self.sigma).Gram_matrix(X, Y)


def timed(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=100)
    ap.add_argument("--T", type=int, default=10)
    ap.add_argument("--d", type=int, default=2)
    ap.add_argument("--order", type=int, default=4)
    ap.add_argument("--h", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    X = synthetic_inputs(a.N, a.T, a.d)[0].to(dev).double()
    G = sk.RBFKernel(a.h).Gram_matrix(X, X).reshape(a.N * a.N, a.T, a.T).contiguous()
    res = {"shape": [a.N, a.T, a.d], "order": a.order}
    res["pde_fwd"] = timed(lambda: ops.pde_fwd(G, a.order), a.reps)
    res["pde_fwd_bwd"] = timed(lambda: ops.pde_fwd_bwd(G, a.order), a.reps)
    res["generic_ordered"] = timed(lambda: ops.gram_fwd_bwd(X, X, 1.0 / a.h, a.order, force_generic=True), a.reps)
    res["generic_sym"] = timed(lambda: ops.gram_fwd_bwd(X, X, 1.0 / a.h, a.order, y_is_x=True, force_generic=True), a.reps)
    k = sk.SigKernel(_GramOnlyRBF(a.h), a.order)
    res["user_gram_and_grad"] = timed(lambda: k.gram_and_grad(X), a.reps)
    print(json.dumps({k_: (round(v, 4) if isinstance(v, float) else v) for k_, v in res.items()}))


if __name__ == "__main__":
    main()
