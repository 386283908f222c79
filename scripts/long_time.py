"""Time the long-path route of the built-in static kernels (csrc/gram_long.hip) next to the user static-kernel route on the
same inputs.

    python scripts/long_time.py [--reps 10]

Prints one JSON line per shape: milliseconds per launch, [median, min, max] of `reps` timed with device events after
warm-up, of
  long_fwd_bwd          ops.gram_long_fwd_bwd(X, X): K and the gradient, the static kernel evaluated inside the sweep,
                        every ordered pair solved;
  long2_y_is_x          ops.gram_long_fwd_bwd2(X, X, y_is_x=True): the same K and gradient, each unordered pair once;
  long_fwd, long2_y_is_x_fwd   the two forward-only launches;
  long_two_ordered      ops.gram_long_fwd_bwd(X, Y, W) then ops.gram_long_fwd_bwd(Y, X, W^T): both slots' gradients from
                        two ordered launches;
  long2_two_slot        ops.gram_long_fwd_bwd2(X, Y, W): both from one launch;
  user_gram_and_grad    SigKernel(<RBF behind Gram_matrix only>).gram_and_grad(X, X): torch builds the [A, B, T, T] grid,
                        sig_pde.hip solves it, torch autograd chains dG to X (the first two shapes).
Shapes: A = B = 32, T = 512, d = 4, order 0; A = B = 16, T = 200, d = 3, order 2; A = B = 64, T = 300, d = 7, order 0 (all
refused by the fused kernels).
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
    return [round(ts[len(ts) // 2], 4), round(ts[0], 4), round(ts[-1], 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--h", type=float, default=1.0)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    for (N, T, d, order, user) in [(32, 512, 4, 0, True), (16, 200, 3, 2, True), (64, 300, 7, 0, False)]:
        X = (torch.randn(N, T, d, generator=g, dtype=torch.float64) / T**0.5).cumsum(1).to(dev)
        Y = (torch.randn(N, T, d, generator=g, dtype=torch.float64) / T**0.5).cumsum(1).to(dev)
        W = torch.rand(N, N, generator=g, dtype=torch.float64).to(dev) + 0.5
        Wt = W.T.contiguous()
        assert not ops.gram_takes(N, N, T, d, order)
        ih = 1.0 / a.h
        res = {"shape": [N, T, d], "order": order}
        res["long_fwd_bwd"] = timed(lambda: ops.gram_long_fwd_bwd(X, X, ih, order), a.reps)
        res["long2_y_is_x"] = timed(lambda: ops.gram_long_fwd_bwd2(X, X, ih, order, y_is_x=True), a.reps)
        res["long_fwd"] = timed(lambda: ops.gram_long_fwd(X, X, ih, order), a.reps)
        res["long2_y_is_x_fwd"] = timed(lambda: ops.gram_long_fwd_bwd2(X, X, ih, order, y_is_x=True, want_gradX=False,
                                                                       want_gradY=False), a.reps)
        res["long_two_ordered"] = timed(lambda: (ops.gram_long_fwd_bwd(X, Y, ih, order, grad_out=W),
                                                 ops.gram_long_fwd_bwd(Y, X, ih, order, grad_out=Wt)), a.reps)
        res["long2_two_slot"] = timed(lambda: ops.gram_long_fwd_bwd2(X, Y, ih, order, grad_out=W), a.reps)
        if user:  # (the third shape's grid and its autograd copies are several GB)
            k = sk.SigKernel(_GramOnlyRBF(a.h), order)
            res["user_gram_and_grad"] = timed(lambda: k.gram_and_grad(X, X), a.reps)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
