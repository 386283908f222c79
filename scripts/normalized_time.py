"""Time the normalised kernel and its gradient from one flagged launch (SIGSVGD_FLAG_NORMALIZED) against
the same result composed from the existing launches, in the sequence `sigkernel._SigKernelNormGram` issues.

    python scripts/normalized_time.py [--reps 10] [--rounds 2]

A = B = 64 paths of T = 300 points, d = 3, order 0, RBF, fp64 I/O, one batch in both slots (Y_IS_X) with the row gradient, a
smooth batch (steps of 0.3 / sqrt(T): every K is positive).  The composition, all on the long route:

    l        = gram_long_fwd_bwd2(X, X, y_is_x, forward only, log_k)            a log-domain forward Gram
    a        = pair_fwd(X, X, log_k)                                            the diagonals
    K^       = exp(l - a_i / 2 - a_j / 2),   U = W K^                           (torch, on the device)
    g        = gram_long_fwd_bwd2(X, X, U, y_is_x, log_k)                       a second Gram launch, with the reverse sweeps
    pX, pY   = pair_fwd_bwd(X, X, -U.sum(1) / 2, log_k)                         the diagonals' gradients
    gradient = g + pX + pY

Milliseconds per call, [median, min, max] of `reps` timed with device events after warm-up, in `rounds` alternating rounds
(composition, flagged, composition, flagged, ...).  One JSON line per round.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from sigsvgd_amd import ops  # noqa: E402


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


def composed(X, W):
    """(K^, first-slot gradient of sum(W K^) at fixed second slot) from the existing launches"""
    fwd = dict(want_gradX=False, want_gradY=False)
    l = ops.gram_long_fwd_bwd2(X, X, 1.0, 0, y_is_x=True, log_k=True, **fwd)[0]
    a = ops.pair_fwd(X, X, 1.0, 0, log_k=True)
    Kh = torch.exp(l - 0.5 * a[:, None] - 0.5 * a[None, :])
    U = W * Kh
    g = ops.gram_long_fwd_bwd2(X, X, 1.0, 0, grad_out=U, y_is_x=True, log_k=True)[1]
    _, pX, pY = ops.pair_fwd_bwd(X, X, 1.0, 0, grad_out=-0.5 * U.sum(1), log_k=True)
    return Kh, g + pX + pY


def flagged(X, W):
    return ops.gram_long_fwd_bwd2(X, X, 1.0, 0, grad_out=W, y_is_x=True, normalized=True)[:2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--A", type=int, default=64)
    ap.add_argument("--T", type=int, default=300)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    A, T, d = a.A, a.T, 3
    g = torch.Generator().manual_seed(0)
    X = (0.3 * torch.randn(A, T, d, generator=g, dtype=torch.float64) / T**0.5).cumsum(1).to(dev)
    W = (torch.rand(A, A, generator=g, dtype=torch.float64) + 0.5).to(dev)
    # the two compute one thing
    Kc, gc = composed(X, W)
    Kf, gf = flagged(X, W)
    dev_K = float(((Kf - Kc).abs() / Kc.abs()).max())
    dev_g = float((gf - gc).abs().max() / gc.abs().max())
    print(json.dumps({"shape": [A, T, d], "Khat_range": [float(Kc.min()), float(Kc.max())], "Khat_off_composition": dev_K,
                      "gradient_off_composition": dev_g,
                      "diagonal_is_one": bool((Kf.diagonal() == 1.0).all())}), flush=True)
    # (the composition solves a diagonal pair's two gradient terms in two launches, and they cancel only to the fp32 rounding of
    #  the stored S; the flagged launch leaves both out: the gradients agree to the long route's bound, not to fp64 rounding)
    assert dev_K < 1e-12 and dev_g < 1e-5, (dev_K, dev_g)
    for r in range(a.rounds):
        res = {"round": r}
        res["composition"] = timed(lambda: composed(X, W), a.reps)
        res["flagged"] = timed(lambda: flagged(X, W), a.reps)
        res["flagged_forward_only"] = timed(lambda: ops.gram_long_fwd_bwd2(X, X, 1.0, 0, y_is_x=True, want_gradX=False,
                                                                           want_gradY=False, normalized=True), a.reps)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
