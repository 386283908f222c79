"""Time the paired signature kernel, `SigKernel.compute_kernel` (the paired mode of csrc/gram_long.hip), next to the route it
replaces for the built-in static kernels, the diagonal of a Gram launch.

    python scripts/pair_time.py [--reps 10]
    python scripts/pair_time.py --modes [--only A,T,d,order]

Prints one JSON line per shape and route: milliseconds per call (median of `reps` timed with device events after warm-up) of
  fwd        the forward alone (no input requires grad);
  fwd_grad   forward and gradient: X and Y require grad, K.sum() is differentiated with respect to both.
Routes: "pair" is compute_kernel(X, Y); "gram_diag" is compute_Gram(X, Y).diagonal(), called explicitly (what compute_kernel
returned before: A^2 solves, and with a gradient a ones-weighted launch in the forward and a second launch in the backward,
whose weights are not uniform; Y gets no gradient there).
Shapes: A = 1024, T = 64, d = 7, order 0 in fp32 and fp64 (SVGD's C4 batch); A = 100, T = 10, d = 2, order 4 (notebook);
A = 6, T = 100, d = 3, order 3 (the reference's arm-spline example) and A = 16 (the edge of compute_kernel's rule for small
forward-only calls); A = 32, T = 1024, d = 4, order 0 (long).  The "pair" line also gives
"pair_fwd_op": `ops.pair_fwd` itself, which compute_kernel's forward passes over where that rule sends it to the diagonal.

--modes times the two schedules of the paired launch instead: `ops.pair_fwd` and `ops.pair_fwd_bwd`
under SIGSVGD_PAIR_MODE=serial (one wavefront per pair) and =bands (a workgroup per pair) in one process, the two modes
alternating call by call, median and min - max of `reps` calls each after warm-up, one JSON line per shape with the waves
per pair of the bands plan and what the default rule picks.  --only A,T,d,order: that shape alone, with whatever schedule the
environment gives (for runs of two builds side by side, SIGSVGD_LIB_PATH).
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import sigsvgd_amd.sigkernel as sk  # noqa: E402
from sigsvgd_amd import ops  # noqa: E402

SHAPES = [(1024, 64, 7, 0, torch.float32), (1024, 64, 7, 0, torch.float64), (100, 10, 2, 4, torch.float32),
          (6, 100, 3, 3, torch.float32), (16, 100, 3, 3, torch.float32), (32, 1024, 4, 0, torch.float32)]


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
    return ts[len(ts) // 2], ts[0], ts[-1]


# (A, T, d, order) of --modes: few long pairs, the reference's refined shapes, and many short pairs (one band: serial always)
MODE_SHAPES = [(1, 4096, 4, 0), (2, 1024, 4, 0), (6, 1024, 4, 0), (32, 1024, 4, 0), (128, 1024, 4, 0), (512, 1024, 4, 0),
               (6, 100, 3, 3), (16, 100, 3, 3), (64, 200, 3, 2), (1024, 64, 7, 0)]
# shapes on both sides of the default rule, timed after them: more pairs than the device holds
# workgroups, few bands per pair, many short pairs of two bands
EDGE_SHAPES = [(700, 1024, 4, 0), (2048, 1024, 4, 0), (2, 700, 2, 0), (2, 450, 3, 0), (2, 386, 3, 0), (2, 322, 3, 0),
               (300, 322, 3, 0), (3, 130, 2, 0), (2000, 100, 3, 0)]


def timed_alternating(fns, reps, warmup=2):
    """{name: (median, min, max)} ms of the calls `fns[name]()`, the names taking turns call by call"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[name].append(a.elapsed_time(b))
    return {name: (sorted(v)[len(v) // 2], min(v), max(v)) for name, v in ts.items()}


def modes(a, dev, g):
    shapes = [tuple(int(v) for v in a.only.split(","))] if a.only else MODE_SHAPES + EDGE_SHAPES
    fixed = ["env"] if a.only else ["serial", "bands"]
    for (A, T, d, order) in shapes:
        X = (torch.randn(A, T, d, generator=g, dtype=torch.float64) / T**0.5).cumsum(1).to(dev, torch.float32)
        Y = (torch.randn(A, T, d, generator=g, dtype=torch.float64) / T**0.5).cumsum(1).to(dev, torch.float32)

        def under(mode, fn):
            def call():
                if mode != "env":
                    os.environ["SIGSVGD_PAIR_MODE"] = mode
                return fn()
            return call

        res = {"shape": [A, T, d], "order": order}
        if not a.only:
            os.environ["SIGSVGD_PAIR_MODE"] = "bands"
            res["waves_per_pair"], res["grid"], res["lds"] = ops.pair_schedule(A, T, T, d, order)
            del os.environ["SIGSVGD_PAIR_MODE"]
            res["default_waves"] = ops.pair_schedule(A, T, T, d, order)[0]
        fwd = timed_alternating({m: under(m, lambda: ops.pair_fwd(X, Y, 1.0 / a.sigma, order)) for m in fixed}, a.reps)
        bwd = timed_alternating({m: under(m, lambda: ops.pair_fwd_bwd(X, Y, 1.0 / a.sigma, order)) for m in fixed}, a.reps)
        if not a.only:
            os.environ.pop("SIGSVGD_PAIR_MODE", None)
        for m in fixed:
            res[m] = {"fwd": [round(v, 4) for v in fwd[m]], "fwd_bwd": [round(v, 4) for v in bwd[m]]}
        print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sigma", type=float, default=1.0)
    ap.add_argument("--modes", action="store_true")
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    if a.modes or a.only:
        return modes(a, dev, g)
    k = sk.SigKernel(sk.RBFKernel(a.sigma), 0)
    for (A, T, d, order, dtype) in SHAPES:
        k.dyadic_order = order
        X = (torch.randn(A, T, d, generator=g, dtype=torch.float64) / T**0.5).cumsum(1).to(dev, dtype)
        Y = (torch.randn(A, T, d, generator=g, dtype=torch.float64) / T**0.5).cumsum(1).to(dev, dtype)
        Xg, Yg = X.clone().requires_grad_(True), Y.clone().requires_grad_(True)
        routes = {"pair": lambda P, Q: k.compute_kernel(P, Q), "gram_diag": lambda P, Q: k.compute_Gram(P, Q).diagonal()}
        for name, route in routes.items():
            def fwd_grad():
                Xg.grad = Yg.grad = None
                route(Xg, Yg).sum().backward()

            res = {"shape": [A, T, d], "order": order, "dtype": str(dtype).replace("torch.", ""), "route": name}
            with torch.no_grad():
                res["fwd"], res["fwd_min"], res["fwd_max"] = timed(lambda: route(X, Y), a.reps)
            res["fwd_grad"], res["fwd_grad_min"], res["fwd_grad_max"] = timed(fwd_grad, a.reps)
            if name == "pair":
                res["pair_fwd_op"], res["pair_fwd_op_min"], res["pair_fwd_op_max"] = timed(
                    lambda: ops.pair_fwd(X, Y, 1.0 / a.sigma, order), a.reps)
            print(json.dumps({k_: (round(v, 4) if isinstance(v, float) else v) for k_, v in res.items()}), flush=True)


if __name__ == "__main__":
    main()
