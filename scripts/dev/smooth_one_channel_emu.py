"""Precision experiment (numpy emulation, CPU): which storage holds the gradient of very smooth one-channel paths at order 0?

Regime of profiles/r04_smooth_one_channel.txt: d = 1, step 0.01-0.02, h = 10 -- K = 1 + O(1e-4) in every pair and the 4-corner
scatter R (a second difference of S = K_fwd * U) is ~1e-5, so the fp32 rounding of values next to 1 is what counts.  Every
scheme sweeps in fp64 (the fp32 sweeps of the register-resident / quadrant kernels add their own error on top of "f32"); the
gradient is assembled in fp64 from each scheme's S.
  f32    : increments, K_fwd, U and S stored fp32 (the register-resident and quadrant kernels' storage)
  cov    : fp64 increments and S, K_fwd stored fp32 (the coverage kernel, T <= 92)
  covbig : fp64 increments, K_fwd and S stored fp32 (the coverage kernel's long-path layout, T > 92)
  cov-1  : as cov, K_fwd - 1 stored fp32
  covbig-1 : as covbig, K_fwd - 1 and S - 1 stored fp32
Errors: gradient error over its largest entry against the all-fp64 oracle, symmetric orientation, grad_out = 1.
usage: python scripts/dev/smooth_one_channel_emu.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from oracle import sigkernel_oracle as O  # noqa: E402  (dev experiment: oracle as the checker)

f32 = np.float32


def r32(a, ofs=0.0):
    return (np.asarray(a) - ofs).astype(f32).astype(np.float64) + ofs


def grad_from_S(X, G, S, h):
    A, T = X.shape[0], X.shape[1]
    R = np.zeros((A, A, T, T))
    R[:, :, 1:, 1:] += S
    R[:, :, :-1, :-1] += S
    R[:, :, 1:, :-1] -= S
    R[:, :, :-1, 1:] -= S
    return np.einsum("ijmn,ijmnc->imc", R, O.static_grad_x(X, X, G, O.RBF, h))


def run(A, T, d, scale, h, seed):
    rng = np.random.default_rng(seed)
    X = np.cumsum(scale * rng.standard_normal((A, T, d)), axis=1).astype(f32)
    _, gref = O.gram_backward(X, X, None, O.RBF, h, 0)
    G = O.static_gram(X, X, O.RBF, h)
    D = O.increments(G)
    out = {}
    for name in ("f32", "cov", "covbig", "cov-1", "covbig-1"):
        g = r32(D) if name == "f32" else D
        Kf = O.pde_sweep(g)
        U = O.pde_sweep(g[..., ::-1, ::-1])[..., ::-1, ::-1][..., 1:, 1:]
        Kf = Kf[..., :-1, :-1]
        ofs = 1.0 if name.endswith("-1") else 0.0
        Kf = r32(Kf, ofs)
        if name == "f32":
            S = r32(Kf * r32(U))
        elif name.startswith("covbig"):
            S = r32(Kf * U, ofs)
        else:
            S = Kf * U
        gr = grad_from_S(X, G, S, h)
        out[name] = np.abs(gr - gref).max() / np.abs(gref).max()
    print(f"A={A} T={T} d={d} scale={scale} h={h} seed={seed}: " + "  ".join(f"{k} {v:.1e}" for k, v in out.items()),
          flush=True)


if __name__ == "__main__":
    for (A, T, d, scale, h) in [(20, 33, 1, 0.01, 10.0), (20, 20, 1, 0.02, 10.0), (12, 128, 1, 0.01, 10.0),
                                (20, 64, 1, 0.01, 10.0), (12, 100, 1, 0.01, 10.0), (20, 33, 2, 0.01, 10.0)]:
        for seed in range(int(sys.argv[1]) if len(sys.argv) > 1 else 2):
            run(A, T, d, scale, h, 100 * T + 10 * d + seed)
