"""Time the median of the point distances on the device, `ops.path_sqdist_select` (csrc/sqdist_select.hip), next to the route
it replaces for the default bandwidth: the [A, B, T, T] fp64 tensor of `sigkernel.gram_sqdist` and `torch.median` of it.

    python scripts/median_time.py [--reps 10] [--shapes C4,long]

Prints one JSON line per shape: milliseconds per call (median, minimum and maximum of `reps` timed with device events after
warm-up) of
  select        ops.path_sqdist_select(X, Y), two buffers;
  select_yx     ops.path_sqdist_select(X), one buffer in both slots (each unordered pair once);
  torch         torch.median(gram_sqdist(X.double(), X.double())), where the tensor is within the 4 GiB the torch route
                forms (the scalar's read-back, which that route also pays, is not timed on either side);
and `passes` / `passes_yx`, the passes of the select that recomputed the distances, `n` the number of elements, and `agree`:
whether the torch median lies within the rounding of the two distance forms of the select's.
Shapes (N, T, d): C1 (16, 20, 2), the notebook's (100, 10, 2), C2 (128, 32, 7), (256, 64, 7) -- the largest bench-like shape
the torch route takes --, C3 (512, 64, 3), C4 (1024, 64, 7), and long paths (16, 2000, 2).
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import sigsvgd_amd.sigkernel as sk  # noqa: E402
from oracle import sigkernel_oracle as O  # noqa: E402
from sigsvgd_amd import ops  # noqa: E402

SHAPES = {"C1": (16, 20, 2), "notebook": (100, 10, 2), "C2": (128, 32, 7), "N256": (256, 64, 7), "C3": (512, 64, 3),
          "C4": (1024, 64, 7), "long": (16, 2000, 2)}


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
    ap.add_argument("--shapes", default=",".join(SHAPES))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for name in a.shapes.split(","):
        N, T, d = SHAPES[name]
        X = O.synthetic_inputs(N, T, d)[0].to(dev)
        Y = X.clone()
        n = N * N * T * T
        res = {"shape": name, "N": N, "T": T, "d": d, "n": n}
        res["select"] = timed(lambda: ops.path_sqdist_select(X, Y), a.reps)
        res["passes"] = ops.path_sqdist_select_passes(dev)
        res["select_yx"] = timed(lambda: ops.path_sqdist_select(X), a.reps)
        res["passes_yx"] = ops.path_sqdist_select_passes(dev)
        m = float(ops.path_sqdist_select(X))
        res["median"] = m
        if n * 8 <= sk._MAX_DIST_BYTES:
            Xd = X.double()
            res["torch"] = timed(lambda: torch.median(sk.gram_sqdist(Xd, Xd)), a.reps)
            mt = float(torch.median(sk.gram_sqdist(Xd, Xd)))
            res["agree"] = abs(mt - m) <= 8 * (d + 3) * 2.0**-53 * float((Xd**2).sum(-1).max())
            torch.cuda.empty_cache()
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
