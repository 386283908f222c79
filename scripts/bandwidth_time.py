"""Time the long route's launches with and without the bandwidth derivative (DESIGN.md section 5.16,
profiles/bandwidth_grad.txt).

    python scripts/bandwidth_time.py [--reps 10] [--tree DIR] [--label NAME]

Prints one JSON line per shape: milliseconds per call, [median, min, max] of `reps` calls timed with device events after
warm-up, of
  gram (A = B = 32, T = 300, d = 3, order 0, fp64):  `ops.gram_long_fwd_bwd2` forward only, with gX, with gX and gY, and
      `ops.gram_long_fwd_bwd_h` with no coordinate gradient, with gX, with gX and gY;
  pair (A = 1024, T = 64, d = 7, order 0, fp32):  `ops.pair_fwd`, `ops.pair_fwd_bwd` (gX and gY), and `ops.pair_fwd_bwd_h`
      with no coordinate gradient and with both.
--tree DIR imports the package from DIR instead of this checkout (a build of another commit: the launches it lacks are left
out), so that two builds can take turns, a process each.
"""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--label", default="")
args = ap.parse_args()
sys.path.insert(0, args.tree)

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
    return [round(t, 4) for t in (ts[len(ts) // 2], ts[0], ts[-1])]


def walks(A, T, d, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    return torch.cumsum(0.05 * torch.randn(A, T, d, generator=g, dtype=torch.float64), dim=1).to(dtype).cuda()


def main():
    has_h = hasattr(ops, "gram_long_fwd_bwd_h")
    A, T, d = 32, 300, 3
    X, Y = walks(A, T, d, 0, torch.float64), walks(A, T, d, 5, torch.float64)
    out = {"label": args.label, "shape": "gram", "A": A, "B": A, "T": T, "d": d, "order": 0, "dtype": "fp64"}
    out["fwd"] = timed(lambda: ops.gram_long_fwd_bwd2(X, Y, 1.0, want_gradX=False, want_gradY=False), args.reps)
    out["fwd_bwd2 gX"] = timed(lambda: ops.gram_long_fwd_bwd2(X, Y, 1.0, want_gradY=False), args.reps)
    out["fwd_bwd2 gX gY"] = timed(lambda: ops.gram_long_fwd_bwd2(X, Y, 1.0), args.reps)
    if has_h:
        out["fwd_bwd_h"] = timed(lambda: ops.gram_long_fwd_bwd_h(X, Y, 1.0, want_gradX=False, want_gradY=False), args.reps)
        out["fwd_bwd_h gX"] = timed(lambda: ops.gram_long_fwd_bwd_h(X, Y, 1.0, want_gradY=False), args.reps)
        out["fwd_bwd_h gX gY"] = timed(lambda: ops.gram_long_fwd_bwd_h(X, Y, 1.0), args.reps)
    print(json.dumps(out), flush=True)

    A, T, d = 1024, 64, 7
    X, Y = walks(A, T, d, 0, torch.float32), walks(A, T, d, 5, torch.float32)
    out = {"label": args.label, "shape": "pair", "A": A, "T": T, "d": d, "order": 0, "dtype": "fp32"}
    out["fwd"] = timed(lambda: ops.pair_fwd(X, Y, 1.0), args.reps)
    out["fwd_bwd gX gY"] = timed(lambda: ops.pair_fwd_bwd(X, Y, 1.0), args.reps)
    if has_h:
        out["fwd_bwd_h"] = timed(lambda: ops.pair_fwd_bwd_h(X, Y, 1.0, want_x=False, want_y=False), args.reps)
        out["fwd_bwd_h gX gY"] = timed(lambda: ops.pair_fwd_bwd_h(X, Y, 1.0), args.reps)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
