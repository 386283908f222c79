"""fp64 numpy reference of the signature kernel with a radial static kernel k = phi(s), s = |x - y|^2 / h, for the kinds the
oracle does not know (IMQ, rational quadratic; RBF too, to tie the helper to `oracle.sigkernel_oracle.gram_backward`).

Built on the oracle's kind-independent pieces (increments, refine, pde_sweep, gg_matrix): G = phi(sqdist / h),
K = pde_sweep(refine(increments(G), n))[..., -1, -1]; S is the block sum of GG over r^2, R its 4-corner scatter (as in
`gram_backward`), and
    gX[i] = sum_j w_ij sum_n R[i,j,m,n] (-2/h) (-phi'(s)) (x_m - y_n),
    gY[j] = sum_i w_ij sum_m R[i,j,m,n] (+2/h) (-phi'(s)) (x_m - y_n).
Paths of X and Y may have different lengths."""
import numpy as np

from oracle import sigkernel_oracle as O

RBF, IMQ, RQ = 0, 2, 3
NAMES = {RBF: "rbf", IMQ: "imq", RQ: "rq"}


def phi(kind: int, s):
    s = np.asarray(s, dtype=np.float64)
    if kind == RBF:
        return np.exp(-s)
    if kind == IMQ:
        return (1.0 + s) ** -0.5
    if kind == RQ:
        return 1.0 / (1.0 + s)
    raise ValueError(kind)


def neg_dphi(kind: int, s):
    """-phi'(s)"""
    k = phi(kind, s)
    if kind == RBF:
        return k
    if kind == IMQ:
        return 0.5 * k**3
    return k**2


def _diff(X, Y):
    X = np.asarray(X, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    return X[:, None, :, None, :] - Y[None, :, None, :, :]  # [A,B,TX,TY,d]


def sqdist(X, Y):
    d = _diff(X, Y)
    return (d * d).sum(-1)


def static_gram(X, Y, kind, h=1.0):
    return phi(kind, sqdist(X, Y) / float(h))


def _solve(X, Y, kind, h, n):
    """-> (K [A,B], R [A,B,TX,TY] = d sum(K) / dG per pair, diff, s)"""
    diff = _diff(X, Y)
    s = (diff * diff).sum(-1) / float(h)
    g = O.refine(O.increments(phi(kind, s)), n)
    K_full = O.pde_sweep(g)
    GG = O.gg_matrix(K_full, g)
    A, B, TX, TY = s.shape
    r = 2**n
    S = GG.reshape(A, B, TX - 1, r, TY - 1, r).sum(axis=(3, 5)) / float(r * r)
    R = np.zeros((A, B, TX, TY))
    R[:, :, 1:, 1:] += S
    R[:, :, :-1, :-1] += S
    R[:, :, 1:, :-1] -= S
    R[:, :, :-1, 1:] -= S
    return K_full[..., -1, -1], R, diff, s


def gram(X, Y, kind, h=1.0, n=0):
    return _solve(X, Y, kind, h, n)[0]


def gram_backward(X, Y, w=None, kind=IMQ, h=1.0, n=0, sym=False):
    """-> (K [A,B], gX [A,TX,d], gY [B,TY,d]) for weights w [A,B] (ones when None); sym: w + w^T (A == B)."""
    K, R, diff, s = _solve(X, Y, kind, h, n)
    w = np.ones(K.shape) if w is None else np.asarray(w, dtype=np.float64)
    if sym:
        w = w + w.T
    core = (w[:, :, None, None] * R * neg_dphi(kind, s))[..., None] * diff * (2.0 / float(h))  # [A,B,TX,TY,d]
    return K, -core.sum(axis=(1, 3)), core.sum(axis=(0, 2))


def pair_backward(X, Y, w=None, kind=IMQ, h=1.0, n=0):
    """-> (K [A], gX [A,TX,d], gY [A,TY,d]) of the pairs (X_i, Y_i), weights w [A]"""
    A = len(X)
    w = np.ones(A) if w is None else np.asarray(w, dtype=np.float64)
    out = [gram_backward(X[i:i + 1], Y[i:i + 1], w[i].reshape(1, 1), kind, h, n) for i in range(A)]
    return (np.array([o[0][0, 0] for o in out]), np.concatenate([o[1] for o in out]), np.concatenate([o[2] for o in out]))


def separated_bundles(offset=30.0, n_each=4, T=16, d=2):
    """Two bundles of smooth paths, the second shifted by `offset` in every coordinate (fp32 values, as fp64)."""
    t = np.linspace(0.0, 1.0, T)[None, :, None]
    k = np.arange(2 * n_each, dtype=np.float64)[:, None, None]
    c = np.arange(d, dtype=np.float64)[None, None, :]
    X = 0.5 * np.sin(2.0 * t * (1.0 + 0.3 * k) + 0.7 * c) + 0.1 * k * t
    X[n_each:] += offset
    return X.astype(np.float32).astype(np.float64)
