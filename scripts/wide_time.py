"""Time RBF paths of 17 to 32 channels on the register-resident kernel's 32-channel layout against the route they take without
the opt-in.

    python scripts/wide_time.py [--reps 10]

Prints one JSON line per size N = 256 and N = 1024 at T = 64, order 0, Y = X: milliseconds per Gram + gradient launch,
[median, min, max] of `reps` timed with device events after warm-up, all in this one process, for
  d = 17 and d = 32 with `fp32_sweeps=True` (csrc/gram_fast_wide.hip) and without it (the coverage kernel: the parent's route),
  d = 16 on the 16-channel layout (the default route; informational: the cost per channel),
and per d "beats": the flagged median is below the unflagged one by more than the larger of the two min-max ranges (the condition
of section 5.18), and "agree": the flagged K per entry and gradient relative to its largest entry against the unflagged launch's."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from sigsvgd_amd import ops  # noqa: E402
from long_time import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    for N in (256, 1024):
        T = 64
        res = {"route": "wide against coverage", "shape": [N, T], "order": 0}
        X16 = (torch.randn(N, T, 16, generator=g, dtype=torch.float64) / T**0.5).cumsum(1).float().to(dev)
        res["d16_fast"] = timed(lambda: ops.gram_fwd_bwd(X16, X16, 1.0, 0, y_is_x=True), a.reps)
        for d in (17, 32):
            X = (torch.randn(N, T, d, generator=g, dtype=torch.float64) / T**0.5).cumsum(1).float().to(dev)
            wide = timed(lambda: ops.gram_fwd_bwd(X, X, 1.0, 0, y_is_x=True, fp32_sweeps=True), a.reps)
            cov = timed(lambda: ops.gram_fwd_bwd(X, X, 1.0, 0, y_is_x=True), a.reps)
            Kw, gw = ops.gram_fwd_bwd(X, X, 1.0, 0, y_is_x=True, fp32_sweeps=True)
            Kc, gc = ops.gram_fwd_bwd(X, X, 1.0, 0, y_is_x=True)
            res[f"d{d}_wide"], res[f"d{d}_coverage"] = wide, cov
            res[f"d{d}_beats"] = bool(cov[0] - wide[0] > max(wide[2] - wide[1], cov[2] - cov[1]))
            res[f"d{d}_agree"] = {"K": float(((Kw - Kc).abs() / Kc.abs()).max()), "grad": float((gw - gc).abs().max() / gc.abs().max())}
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
