"""Time the two-sided gradient launch of the long route with and without SIGSVGD_FLAG_LOG_K.

    python scripts/log_k_time.py [--reps 10] [--rounds 2]

A = B = 64 paths of T = 300 points, d = 3, order 0, RBF, fp64 I/O, a smooth batch (steps of 0.3 / sqrt(T): every K is
positive and nothing would overflow, so both launches do the same arithmetic and the difference is the cost of the flag); `ops.gram_long_fwd_bwd2(X, Y, W)`
with both gradients, and the forward-only launch.  Milliseconds per launch, [median, min, max] of `reps` timed with device
events after warm-up, in `rounds` alternating rounds (unflagged, flagged, unflagged, flagged, ...).  One JSON line per round.
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
    Y = (0.3 * torch.randn(A, T, d, generator=g, dtype=torch.float64) / T**0.5).cumsum(1).to(dev)
    W = (torch.rand(A, A, generator=g, dtype=torch.float64) + 0.5).to(dev)
    # the two launches compute one thing
    K, gX, gY = ops.gram_long_fwd_bwd2(X, Y, 1.0, 0, grad_out=W / ops.gram_long_fwd_bwd2(X, Y, 1.0, 0, want_gradX=False,
                                                                                       want_gradY=False)[0])
    L, lX, lY = ops.gram_long_fwd_bwd2(X, Y, 1.0, 0, grad_out=W, log_k=True)
    dev_ln = float(((L - K.log()).abs() / L.abs().clamp(min=1.0)).max())
    dev_g = max(float((lX - gX).abs().max() / gX.abs().max()), float((lY - gY).abs().max() / gY.abs().max()))
    print(json.dumps({"shape": [A, T, d], "K_range": [float(K.min()), float(K.max())], "ln_K_off_log_K": dev_ln,
                      "gradient_off_unflagged_over_K": dev_g}), flush=True)
    assert dev_ln <= 1e-13 and dev_g < 1e-5, (dev_ln, dev_g)
    fwd = dict(want_gradX=False, want_gradY=False)
    for r in range(a.rounds):
        res = {"round": r}
        res["grad_unflagged"] = timed(lambda: ops.gram_long_fwd_bwd2(X, Y, 1.0, 0, grad_out=W), a.reps)
        res["grad_log_k"] = timed(lambda: ops.gram_long_fwd_bwd2(X, Y, 1.0, 0, grad_out=W, log_k=True), a.reps)
        res["fwd_unflagged"] = timed(lambda: ops.gram_long_fwd_bwd2(X, Y, 1.0, 0, **fwd), a.reps)
        res["fwd_log_k"] = timed(lambda: ops.gram_long_fwd_bwd2(X, Y, 1.0, 0, log_k=True, **fwd), a.reps)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
