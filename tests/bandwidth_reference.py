"""fp64 numpy reference of the derivative of the signature kernel in the static kernel's bandwidth,
shared by tests/test_bandwidth_grad_cpu.py and tests/test_gpu_bandwidth_grad.py.

k = phi(s), s = |x - y|^2 / h.  With R = d sum(K) / dG per pair (the 4-corner scatter of the block sums of GG: the reference's
GG convention),
    dK/dh = sum_{m,n} R[m][n] (-phi'(s)) s / h,        dK/d(1/h) = -h^2 dK/dh.
The default stencil takes R from `radial_reference._solve`; the first-order stencil, for which GG is the exact adjoint, builds
the same R from the oracle's pieces (tests/test_bandwidth_grad_cpu.py holds that one to a central difference of K)."""
import numpy as np

import radial_reference as RR
from oracle import sigkernel_oracle as O


def scatter(S):
    A, B, M, N = S.shape
    R = np.zeros((A, B, M + 1, N + 1))
    R[:, :, 1:, 1:] += S
    R[:, :, :-1, :-1] += S
    R[:, :, 1:, :-1] -= S
    R[:, :, :-1, 1:] -= S
    return R


def dK_dh(X, Y, kind, h, n, naive=False):
    """[A, B]: every pair's dK/dh"""
    if not naive:
        _, R, _, s = RR._solve(X, Y, kind, h, n)
    else:
        assert kind == RR.RBF  # (the oracle's static_gram knows RBF and linear)
        K_full, g, _ = O.gram_forward_full(X, Y, O.RBF, h, n, naive=True)
        GG = O.gg_matrix(K_full, g, True)
        A, B, TX, TY = len(X), len(Y), X.shape[1], Y.shape[1]
        r = 2**n
        R = scatter(GG.reshape(A, B, TX - 1, r, TY - 1, r).sum(axis=(3, 5)) / float(r * r))
        s = RR.sqdist(X, Y) / float(h)
    return (R * RR.neg_dphi(kind, s) * s).sum((2, 3)) / float(h)


def dK_dinvh(X, Y, kind, h, n, naive=False):
    return -float(h) ** 2 * dK_dh(X, Y, kind, h, n, naive)
