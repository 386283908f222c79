"""Time a ragged batch on the long route with and without SIGSVGD_FLAG_NAN_TAILS.

    python scripts/nan_tails_time.py [--reps 10] [--rounds 2]

A = B = 64 paths of up to T = 300 points, d = 3, order 0, RBF, fp64 I/O, lengths seeded uniform in [75, 300]; the two-sided
gradient launch `ops.gram_long_fwd_bwd2(X, Y, W)` with both gradients.  Milliseconds per launch, [median, min, max] of `reps`
timed with device events after warm-up, in `rounds` alternating rounds (a, b, c, a, b, c, ...), of
  a  padded      the unflagged launch on the last-point-padded batches: every pair on the (T - 1)^2 grid;
  b  nan_tails   the flagged launch on the NaN-padded batches: every pair on its own grid;
  c  sorted      the flagged launch with the paths of both batches sorted by length, longest first;
and of the all-full-length batch, unflagged against flagged (the cost of the length pass and the per-pair geometry).
The cell ratio sum_ij (L_i - 1)(L_j - 1) / (A B (T - 1)^2) is printed beside the timings.  One JSON line per round.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
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


def ragged(P, L, fill_last):
    """P [A, T, d] -> the batch whose path i ends at L[i]: its last point repeated, or NaN, from there on"""
    t = torch.arange(P.shape[1], device=P.device)[None, :, None]
    Ld = torch.as_tensor(L, device=P.device)[:, None, None]
    last = P[torch.arange(P.shape[0]), torch.as_tensor(L) - 1][:, None, :]
    return torch.where(t < Ld, P, last if fill_last else torch.full_like(P, float("nan"))).contiguous()


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
    rng = np.random.default_rng(0)
    X = (torch.randn(A, T, d, generator=g, dtype=torch.float64) / T**0.5).cumsum(1).to(dev)
    Y = (torch.randn(A, T, d, generator=g, dtype=torch.float64) / T**0.5).cumsum(1).to(dev)
    W = (torch.rand(A, A, generator=g, dtype=torch.float64) + 0.5).to(dev)
    LX, LY = rng.integers(T // 4, T + 1, A), rng.integers(T // 4, T + 1, A)
    ratio = float(np.outer(LX - 1, LY - 1).sum()) / (A * A * (T - 1) ** 2)
    Xl, Yl, Xn, Yn = ragged(X, LX, True), ragged(Y, LY, True), ragged(X, LX, False), ragged(Y, LY, False)
    ox, oy = np.argsort(-LX, kind="stable"), np.argsort(-LY, kind="stable")
    Xs, Ys = Xn[torch.as_tensor(ox, device=dev)].contiguous(), Yn[torch.as_tensor(oy, device=dev)].contiguous()
    Ws = W[torch.as_tensor(ox, device=dev)][:, torch.as_tensor(oy, device=dev)].contiguous()
    # the three launches compute one thing
    Ka, gXa, _ = ops.gram_long_fwd_bwd2(Xl, Yl, 1.0, 0, grad_out=W)
    Kb, gXb, _ = ops.gram_long_fwd_bwd2(Xn, Yn, 1.0, 0, grad_out=W, nan_tails=True)
    Kc, _, _ = ops.gram_long_fwd_bwd2(Xs, Ys, 1.0, 0, grad_out=Ws, nan_tails=True)
    assert float(((Ka - Kb).abs() / Ka.abs()).max()) < 1e-9
    assert torch.equal(Kc, Kb[torch.as_tensor(ox, device=dev)][:, torch.as_tensor(oy, device=dev)])
    print(json.dumps({"shape": [A, T, d], "lengths": [int(T // 4), T], "cell_ratio": round(ratio, 4)}), flush=True)
    for r in range(a.rounds):
        res = {"round": r}
        res["a_padded"] = timed(lambda: ops.gram_long_fwd_bwd2(Xl, Yl, 1.0, 0, grad_out=W), a.reps)
        res["b_nan_tails"] = timed(lambda: ops.gram_long_fwd_bwd2(Xn, Yn, 1.0, 0, grad_out=W, nan_tails=True), a.reps)
        res["c_sorted"] = timed(lambda: ops.gram_long_fwd_bwd2(Xs, Ys, 1.0, 0, grad_out=Ws, nan_tails=True), a.reps)
        res["full_unflagged"] = timed(lambda: ops.gram_long_fwd_bwd2(X, Y, 1.0, 0, grad_out=W), a.reps)
        res["full_flagged"] = timed(lambda: ops.gram_long_fwd_bwd2(X, Y, 1.0, 0, grad_out=W, nan_tails=True), a.reps)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
