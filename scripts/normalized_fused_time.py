"""Time the normalised kernel and its gradient on the fused Gram route (SIGSVGD_FLAG_NORMALIZED_FUSED)
against the unflagged launch it wraps and against the long route's normalised launch (SIGSVGD_FLAG_NORMALIZED, section 5.22).

    python scripts/normalized_fused_time.py [--reps 10] [--rounds 2] [--N 1024] [--T 64] [--d 7]

The benchmark's shape: N = 1024 paths of T = 64 points, d = 7, order 0, RBF, fp32 I/O, one batch in both slots (Y_IS_X), unit
weights, a smooth batch (steps of 0.05).  Three launches, each returning K (or K^) and the first-slot gradient:

    (a) unflagged   ops.gram_fwd_bwd(X, X, y_is_x)
    (b) flagged     ops.gram_fwd_bwd(X, X, y_is_x, normalized)        diagonal pass, W', (a) under W', finish
    (c) long        ops.gram_long_fwd_bwd2(X, X, y_is_x, normalized)  fp64 log-domain sweeps, each unordered pair once

Milliseconds per call, [median, min, max] of `reps` timed with device events after warm-up, in `rounds` alternating rounds
(a, b, c, a, b, c, ...).  One JSON line per round, with (b) - (a) and (c) / (b) of the medians.
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
    ap.add_argument("--N", type=int, default=1024)
    ap.add_argument("--T", type=int, default=64)
    ap.add_argument("--d", type=int, default=7)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    X = (0.05 * torch.randn(a.N, a.T, a.d, generator=g)).cumsum(1).to(dev)
    unflagged = lambda: ops.gram_fwd_bwd(X, X, 1.0, 0, y_is_x=True)
    flagged = lambda: ops.gram_fwd_bwd(X, X, 1.0, 0, y_is_x=True, normalized=True)
    long_route = lambda: ops.gram_long_fwd_bwd2(X, X, 1.0, 0, y_is_x=True, want_gradY=False, normalized=True)[:2]
    # the two normalised launches compute one thing
    K, _ = unflagged()
    Kf, gf = flagged()
    Kl, gl = long_route()
    off = Kl != 1.0
    print(json.dumps({"shape": [a.N, a.T, a.d], "K_diagonal_range": [float(K.diagonal().min()), float(K.diagonal().max())],
                      "Khat_range": [float(Kl.min()), float(Kl[off].max())],
                      "Khat_fused_off_long": float(((Kf - Kl).abs() / Kl.abs()).max()),
                      "gradient_fused_off_long": float((gf - gl).abs().max() / gl.abs().max()),
                      "diagonal_is_one": bool((Kf.diagonal() == 1.0).all()), "symmetric": bool(torch.equal(Kf, Kf.T))}), flush=True)
    for r in range(a.rounds):
        res = {"round": r}
        res["unflagged"] = timed(unflagged, a.reps)
        res["flagged"] = timed(flagged, a.reps)
        res["long_route"] = timed(long_route, a.reps)
        res["flagged_minus_unflagged_ms"] = round(res["flagged"][0] - res["unflagged"][0], 4)
        res["long_over_flagged"] = round(res["long_route"][0] / res["flagged"][0], 3)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
