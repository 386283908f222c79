"""Time the long-path route of the built-in static kernels (csrc/gram_long.hip) next to the user static-kernel route on the
same inputs.

    python scripts/long_time.py [--reps 10]

Prints one JSON line per shape: milliseconds per launch (median of `reps` timed with device events after warm-up) of
  long_fwd_bwd          ops.gram_long_fwd_bwd(X, X): K and the gradient, the static kernel evaluated inside the sweep;
  user_gram_and_grad    SigKernel(<RBF behind Gram_matrix only>).gram_and_grad(X, X): torch builds the [A, B, T, T] grid,
                        sig_pde.hip solves it, torch autograd chains dG to X.
Shapes: A = B = 32, T = 512, d = 4, order 0; A = B = 16, T = 200, d = 3, order 2 (both refused by the fused kernels).
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from sigsvgd_amd import ops  # noqa: E402
import sigsvgd_amd.sigkernel as sk  # noqa: E402


class _GramOnlyRBF:
    def __init__(self, sigma):
        self.sigma = sigma

    def Gram_matrix(self, X, Y):
        return sk.RBFKernel(self.sigma).Gram_matrix(X, Y)


def timed(fn, reps, warmup=2):
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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--h", type=float, default=1.0)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    for (N, T, d, order) in [(32, 512, 4, 0), (16, 200, 3, 2)]:
        X = (torch.randn(N, T, d, generator=g, dtype=torch.float64) / T**0.5).cumsum(1).to(dev)
        assert not ops.gram_takes(N, N, T, d, order)
        res = {"shape": [N, T, d], "order": order}
        res["long_fwd_bwd"] = timed(lambda: ops.gram_long_fwd_bwd(X, X, 1.0 / a.h, order), a.reps)
        k = sk.SigKernel(_GramOnlyRBF(a.h), order)
        res["user_gram_and_grad"] = timed(lambda: k.gram_and_grad(X, X), a.reps)
        print(json.dumps({k_: (round(v, 4) if isinstance(v, float) else v) for k_, v in res.items()}), flush=True)


if __name__ == "__main__":
    main()
