"""Time the built-in static kernels next to each other on the routes that take all of them.

    python scripts/static_kinds_time.py [--reps 10] [--fp32-sweeps]

Prints one JSON line per shape: milliseconds per Gram + gradient launch, [median, min, max] of `reps` timed with device
events after warm-up, for RBF (the yardstick; on the coverage kernel with force_generic=True, since RBF alone has the
fp32-sweep kernels), IMQ, the rational quadratic kernel and the two Matern kernels:
  coverage kernel  N = 100, T = 10, d = 2, order 4 and N = 256, T = 64, d = 7, order 0: ops.gram_fwd_bwd(X, X, y_is_x=True);
  long route       A = B = 32, T = 512, d = 4, order 0: ops.gram_long_fwd_bwd(X, X).
Next to the first shape: the user route of the same IMQ kernel (torch builds the [N, N, T, T] grid, sig_pde.hip solves it,
autograd chains dG to X) and the peak device memory of both routes.
--fp32-sweeps prints instead, for N = 256 and N = 1024 at T = 64, d = 7, order 0, Y = X, one line with
RBF on the register-resident kernel (the default route), IMQ and the rational quadratic kernel on it (`fp32_sweeps=True`) and
both on the coverage kernel (their default route), all in this one process."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from sigsvgd_amd import _lib, ops  # noqa: E402
import sigsvgd_amd.sigkernel as sk  # noqa: E402
from long_time import timed  # noqa: E402

KINDS = {"rbf": _lib.STATIC_RBF, "imq": _lib.STATIC_IMQ, "rq": _lib.STATIC_RQ, "matern32": _lib.STATIC_MATERN32,
         "matern52": _lib.STATIC_MATERN52}


class _GramOnlyIMQ:
    def __init__(self, sigma):
        self.Gram_matrix = sk.IMQStaticKernel(sigma).Gram_matrix


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2**20, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--fp32-sweeps", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    if a.fp32_sweeps:
        for N in (256, 1024):
            T, d = 64, 7
            X = (torch.randn(N, T, d, generator=g, dtype=torch.float64) / T**0.5).cumsum(1).float().to(dev)
            res = {"route": "fast against coverage", "shape": [N, T, d], "order": 0}
            res["rbf_fast"] = timed(lambda: ops.gram_fwd_bwd(X, X, 1.0, 0, KINDS["rbf"], y_is_x=True), a.reps)
            for name in ("imq", "rq"):
                res[name + "_fast"] = timed(lambda: ops.gram_fwd_bwd(X, X, 1.0, 0, KINDS[name], y_is_x=True, fp32_sweeps=True), a.reps)
            for name in ("imq", "rq"):
                res[name + "_coverage"] = timed(lambda: ops.gram_fwd_bwd(X, X, 1.0, 0, KINDS[name], y_is_x=True), a.reps)
            print(json.dumps(res), flush=True)
        return
    for (N, T, d, order) in [(100, 10, 2, 4), (256, 64, 7, 0)]:
        X = (torch.randn(N, T, d, generator=g, dtype=torch.float64) / T**0.5).cumsum(1).float().to(dev)
        res = {"route": "coverage", "shape": [N, T, d], "order": order}
        for name, kind in KINDS.items():
            assert ops.gram_takes(N, N, T, d, order, kind)
            res[name] = timed(lambda: ops.gram_fwd_bwd(X, X, 1.0, order, kind, y_is_x=True, force_generic=kind == 0), a.reps)
        if T == 10:
            fused, user = sk.SigKernel(sk.IMQStaticKernel(1.0), order), sk.SigKernel(_GramOnlyIMQ(1.0), order)
            res["imq_user_gram_and_grad"] = timed(lambda: user.gram_and_grad(X, X), a.reps)
            res["peak_mb"] = {"imq": peak_mb(lambda: fused.gram_and_grad(X, None)), "imq_user": peak_mb(lambda: user.gram_and_grad(X, X))}
        print(json.dumps(res), flush=True)
    N, T, d = 32, 512, 4
    X = (torch.randn(N, T, d, generator=g, dtype=torch.float64) / T**0.5).cumsum(1).to(dev)
    res = {"route": "long", "shape": [N, T, d], "order": 0}
    for name, kind in KINDS.items():
        assert not ops.gram_takes(N, N, T, d, 0, kind)
        res[name] = timed(lambda: ops.gram_long_fwd_bwd(X, X, 1.0, 0, kind), a.reps)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
