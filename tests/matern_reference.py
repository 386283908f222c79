"""fp64 numpy reference of the signature kernel with a Matern static kernel, shared by
tests/test_matern_cpu.py and tests/test_gpu_matern.py.  k = phi(s), s = |x - y|^2 / h clamped at 0:

    Matern-3/2 (kind 6): u = sqrt(3 s), phi = (1 + u) e^-u,           -phi' = (3/2) e^-u
    Matern-5/2 (kind 7): u = sqrt(5 s), phi = (1 + u + u^2 / 3) e^-u, -phi' = (5/6) (1 + u) e^-u

Built like tests/radial_reference.py on the oracle's kind-independent pieces (increments, refine, pde_sweep, gg_matrix):
G = phi(sqdist / h), K = pde_sweep(refine(increments(G), n))[..., -1, -1]; S is the block sum of GG over r^2, R its 4-corner
scatter, and
    gX[i] = sum_j w_ij sum_n R[i,j,m,n] (-2/h) (-phi'(s)) (x_m - y_n),
    gY[j] = sum_i w_ij sum_m R[i,j,m,n] (+2/h) (-phi'(s)) (x_m - y_n),
    dK_ij / d(1/h) = - sum_{m,n} R[i,j,m,n] (-phi'(s)) |x_m - y_n|^2.
`naive`: the first-order stencil, of which GG is the exact adjoint (the contractions are then derivatives of K).  Paths of X and
Y may have different lengths."""
import numpy as np

from oracle import sigkernel_oracle as O

MATERN32, MATERN52 = 6, 7
KINDS = (MATERN32, MATERN52)
NAMES = {MATERN32: "matern32", MATERN52: "matern52"}


def _u(kind: int, s):
    s = np.maximum(np.asarray(s, dtype=np.float64), 0.0)
    if kind == MATERN32:
        return np.sqrt(3.0 * s)
    if kind == MATERN52:
        return np.sqrt(5.0 * s)
    raise ValueError(kind)


def phi(kind: int, s):
    u = _u(kind, s)
    return (1.0 + u) * np.exp(-u) if kind == MATERN32 else (1.0 + u + u * u / 3.0) * np.exp(-u)


def neg_dphi(kind: int, s):
    """-phi'(s), finite at s = 0 (3/2 and 5/6)"""
    u = _u(kind, s)
    return 1.5 * np.exp(-u) if kind == MATERN32 else (5.0 / 6.0) * (1.0 + u) * np.exp(-u)


def _diff(X, Y):
    X = np.asarray(X, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    return X[:, None, :, None, :] - Y[None, :, None, :, :]  # [A,B,TX,TY,d]


def sqdist(X, Y):
    d = _diff(X, Y)
    return (d * d).sum(-1)


def static_gram(X, Y, kind, h=1.0):
    return phi(kind, sqdist(X, Y) / float(h))


def _solve(X, Y, kind, h, n, naive=False):
    """-> (K [A,B], R [A,B,TX,TY] = d sum(K) / dG per pair, diff, s)"""
    diff = _diff(X, Y)
    s = (diff * diff).sum(-1) / float(h)
    g = O.refine(O.increments(phi(kind, s)), n)
    K_full = O.pde_sweep(g, naive)
    GG = O.gg_matrix(K_full, g, naive)
    A, B, TX, TY = s.shape
    r = 2**n
    S = GG.reshape(A, B, TX - 1, r, TY - 1, r).sum(axis=(3, 5)) / float(r * r)
    R = np.zeros((A, B, TX, TY))
    R[:, :, 1:, 1:] += S
    R[:, :, :-1, :-1] += S
    R[:, :, 1:, :-1] -= S
    R[:, :, :-1, 1:] -= S
    return K_full[..., -1, -1], R, diff, s


def gram(X, Y, kind, h=1.0, n=0, naive=False):
    return _solve(X, Y, kind, h, n, naive)[0]


def gram_backward(X, Y, w=None, kind=MATERN32, h=1.0, n=0, sym=False, naive=False):
    """-> (K [A,B], gX [A,TX,d], gY [B,TY,d]) for weights w [A,B] (ones when None); sym: w + w^T (A == B)."""
    K, R, diff, s = _solve(X, Y, kind, h, n, naive)
    w = np.ones(K.shape) if w is None else np.asarray(w, dtype=np.float64)
    if sym:
        w = w + w.T
    core = (w[:, :, None, None] * R * neg_dphi(kind, s))[..., None] * diff * (2.0 / float(h))  # [A,B,TX,TY,d]
    return K, -core.sum(axis=(1, 3)), core.sum(axis=(0, 2))


def pair_backward(X, Y, w=None, kind=MATERN32, h=1.0, n=0):
    """-> (K [A], gX [A,TX,d], gY [A,TY,d]) of the pairs (X_i, Y_i), weights w [A]"""
    A = len(X)
    w = np.ones(A) if w is None else np.asarray(w, dtype=np.float64)
    out = [gram_backward(X[i:i + 1], Y[i:i + 1], w[i].reshape(1, 1), kind, h, n) for i in range(A)]
    return (np.array([o[0][0, 0] for o in out]), np.concatenate([o[1] for o in out]), np.concatenate([o[2] for o in out]))


def dK_dinvh(X, Y, kind, h=1.0, n=0, naive=False):
    """[A, B]: every pair's dK / d(1/h) = - sum R (-phi'(s)) |x - y|^2"""
    _, R, diff, s = _solve(X, Y, kind, h, n, naive)
    return -(R * neg_dphi(kind, s) * (diff * diff).sum(-1)).sum((2, 3))


def pair_dK_dinvh(X, Y, kind, h=1.0, n=0):
    """[A]: dK / d(1/h) of the pairs (X_i, Y_i)"""
    return np.array([dK_dinvh(X[i:i + 1], Y[i:i + 1], kind, h, n)[0, 0] for i in range(len(X))])
