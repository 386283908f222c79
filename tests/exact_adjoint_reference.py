"""fp64 numpy reference of the EXACT gradient of the discrete signature kernel, shared by
tests/test_exact_adjoint_cpu.py and tests/test_gpu_exact_adjoint.py.

The discrete kernel is K = sol[P][Q] of the sweep K11 = (K10 + K01) A(g) - K00 B(g) on the refined grid, g[p][q] =
D[p >> n][q >> n] / r^2, with A = 1 + g/2 + g^2/12, B = 1 - g^2/12 (default stencil) or A = 1, B = 1 - g (naive).  Its adjoint:

    lambda(p, q) = dK / dK[p+1][q+1]:   lambda(P-1, Q-1) = 1,
    lambda(p, q) = A(g(p, q+1)) lambda(p, q+1) + A(g(p+1, q)) lambda(p+1, q) - B(g(p+1, q+1)) lambda(p+1, q+1)   (0 outside),
    dK / dg(p, q) = lambda(p, q) c(p, q),   c = (K10 + K01) A'(g) - K00 B'(g),
    S[a][b] = r^-2 sum over the block of dK / dg   (= dK / dD[a][b]),

and everything behind S is what the GG references do with their S (tests/radial_reference.py, tests/matern_reference.py,
oracle/sigkernel_oracle.py): the 4-corner scatter R = dK / dG, then the static kernel's own derivatives,

    gX[i] = sum_j w_ij sum_n R[i,j,m,n] dk/dx,   gY[j] = sum_i w_ij sum_m R[i,j,m,n] dk/dy,
    dK_ij / d(1/h) = - sum_{m,n} R[i,j,m,n] (-phi'(s)) |x_m - y_n|^2         (radial kinds, s = |x - y|^2 / h).

With the naive stencil c = K00 and lambda is the oracle's K_rev: the reference's GG convention, which is exact there.  The
static kernels' radial profiles are the existing references' (phi, -phi'); the linear kernel is <x, y>.  Paths of X and Y may
have different lengths."""
import numpy as np

import matern_reference as MR
import radial_reference as RR
from oracle import sigkernel_oracle as O

RBF, LINEAR, IMQ, RQ, MATERN32, MATERN52 = 0, 1, 2, 3, 6, 7
KINDS = (RBF, LINEAR, IMQ, RQ, MATERN32, MATERN52)
RADIAL = (RBF, IMQ, RQ, MATERN32, MATERN52)


def _profile(kind):
    return MR if kind in (MATERN32, MATERN52) else RR


# ---- the PDE and its adjoint on increments ----------------------------------------------------------------------------------
def _coef(g, naive):
    """A, B, A', B' of the stencil at increments g"""
    if naive:
        return np.ones_like(g), 1.0 - g, np.zeros_like(g), -np.ones_like(g)
    return 1.0 + 0.5 * g + g * g / 12.0, 1.0 - g * g / 12.0, 0.5 + g / 6.0, -g / 6.0


def forward(D, n=0, naive=False):
    """coarse increments D [..., M-1, N-1] -> (K_full [..., P+1, Q+1], g [..., P, Q]): the oracle's refinement and sweep"""
    g = O.refine(np.asarray(D, dtype=np.float64), n)
    return O.pde_sweep(g, naive), g


def adjoint(K_full, g, naive=False):
    """-> dK / dg [..., P, Q] by the recurrence of the module docstring, anti-diagonal by anti-diagonal from the far corner"""
    P, Q = g.shape[-2], g.shape[-1]
    A, B, dA, dB = _coef(g, naive)
    lam = np.zeros(g.shape[:-2] + (P + 1, Q + 1))  # (one row and column of zeros: outside the grid)
    alpha = np.zeros_like(lam)
    beta = np.zeros_like(lam)
    for s in range(P + Q - 2, -1, -1):
        p = np.arange(max(0, s - Q + 1), min(P, s + 1))
        q = s - p
        if s == P + Q - 2:
            lam[..., p, q] = 1.0
        else:
            lam[..., p, q] = alpha[..., p, q + 1] + alpha[..., p + 1, q] - beta[..., p + 1, q + 1]
        alpha[..., p, q] = A[..., p, q] * lam[..., p, q]
        beta[..., p, q] = B[..., p, q] * lam[..., p, q]
    c = (K_full[..., 1:, :-1] + K_full[..., :-1, 1:]) * dA - K_full[..., :-1, :-1] * dB
    return lam[..., :P, :Q] * c


def block_sum(dKdg, n):
    """S[..., a, b] = r^-2 sum of dK / dg over block (a, b): dK / dD"""
    r = 2**n
    P, Q = dKdg.shape[-2:]
    lead = dKdg.shape[:-2]
    return dKdg.reshape(lead + (P // r, r, Q // r, r)).sum(axis=(-3, -1)) / float(r * r)


def scatter(S):
    """R[..., m, n] = dK / dG from S = dK / dD: the 4-corner scatter"""
    R = np.zeros(S.shape[:-2] + (S.shape[-2] + 1, S.shape[-1] + 1))
    R[..., 1:, 1:] += S
    R[..., :-1, :-1] += S
    R[..., 1:, :-1] -= S
    R[..., :-1, 1:] -= S
    return R


def pde(G, n=0, naive=False):
    """static-kernel grids G [..., M, N] -> (K [...], dK/dD [..., M-1, N-1], dK/dG [..., M, N])"""
    K_full, g = forward(O.increments(np.asarray(G, dtype=np.float64)), n, naive)
    S = block_sum(adjoint(K_full, g, naive), n)
    return K_full[..., -1, -1], S, scatter(S)


def pde_K_of_D(D, n=0, naive=False):
    return forward(D, n, naive)[0][..., -1, -1]


# ---- the static kernels and the chains to X, Y and 1/h ---------------------------------------------------------------------
def _diff(X, Y):
    X = np.asarray(X, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    return X[:, None, :, None, :] - Y[None, :, None, :, :]  # [A,B,TX,TY,d]


def static_gram(X, Y, kind, h=1.0):
    if kind == LINEAR:
        return np.einsum("ipk,jqk->ijpq", np.asarray(X, np.float64), np.asarray(Y, np.float64))
    d = _diff(X, Y)
    return _profile(kind).phi(kind, (d * d).sum(-1) / float(h))


def gram(X, Y, kind=RBF, h=1.0, n=0, naive=False):
    return pde(static_gram(X, Y, kind, h), n, naive)[0]


def gram_backward(X, Y, w=None, kind=RBF, h=1.0, n=0, sym=False, naive=False):
    """-> (K [A,B], gX [A,TX,d], gY [B,TY,d]) for weights w [A,B] (ones when None); sym: w + w^T (A == B)"""
    K, _, R = pde(static_gram(X, Y, kind, h), n, naive)
    w = np.ones(K.shape) if w is None else np.asarray(w, dtype=np.float64)
    if sym:
        w = w + w.T
    wR = w[:, :, None, None] * R
    if kind == LINEAR:
        return K, np.einsum("ijmn,jnc->imc", wR, np.asarray(Y, np.float64)), np.einsum("ijmn,imc->jnc", wR,
                                                                                       np.asarray(X, np.float64))
    diff = _diff(X, Y)
    s = (diff * diff).sum(-1) / float(h)
    core = (wR * _profile(kind).neg_dphi(kind, s))[..., None] * diff * (2.0 / float(h))
    return K, -core.sum(axis=(1, 3)), core.sum(axis=(0, 2))


def pair_backward(X, Y, w=None, kind=RBF, h=1.0, n=0, naive=False):
    """-> (K [A], gX [A,TX,d], gY [A,TY,d]) of the pairs (X_i, Y_i), weights w [A]"""
    A = len(X)
    w = np.ones(A) if w is None else np.asarray(w, dtype=np.float64)
    out = [gram_backward(X[i:i + 1], Y[i:i + 1], w[i].reshape(1, 1), kind, h, n, False, naive) for i in range(A)]
    return (np.array([o[0][0, 0] for o in out]), np.concatenate([o[1] for o in out]), np.concatenate([o[2] for o in out]))


def dK_dinvh(X, Y, kind=RBF, h=1.0, n=0, naive=False):
    """[A, B]: every pair's dK / d(1/h) = - sum R (-phi'(s)) |x - y|^2 (radial kinds)"""
    R = pde(static_gram(X, Y, kind, h), n, naive)[2]
    diff = _diff(X, Y)
    sq = (diff * diff).sum(-1)
    return -(R * _profile(kind).neg_dphi(kind, sq / float(h)) * sq).sum((2, 3))


def pair_dK_dinvh(X, Y, kind=RBF, h=1.0, n=0, naive=False):
    return np.array([dK_dinvh(X[i:i + 1], Y[i:i + 1], kind, h, n, naive)[0, 0] for i in range(len(X))])


# ---- central differences of the helper's own K (tests only) ------------------------------------------------------------------
def fd_dK_dD(D, n=0, naive=False, eps=1e-6, chunk=512):
    """central differences of K in every coarse increment of ONE grid D [M-1, N-1] (the perturbed grids swept in batches)"""
    D = np.asarray(D, dtype=np.float64)
    out = np.zeros(D.size)
    for e0 in range(0, D.size, chunk):
        idx = np.arange(e0, min(D.size, e0 + chunk))
        Dp = np.repeat(D.reshape(1, -1), len(idx), axis=0)
        Dm = Dp.copy()
        Dp[np.arange(len(idx)), idx] += eps
        Dm[np.arange(len(idx)), idx] -= eps
        both = np.concatenate([Dp, Dm]).reshape((2 * len(idx),) + D.shape)
        K = pde_K_of_D(both, n, naive)
        out[idx] = (K[:len(idx)] - K[len(idx):]) / (2 * eps)
    return out.reshape(D.shape)


def fd_dK_dX(X, Y, kind=RBF, h=1.0, n=0, eps=1e-6):
    """central differences of sum_j K[0, j] in every coordinate of the ONE path X [1, TX, d] (the perturbed paths as a batch)"""
    X = np.asarray(X, dtype=np.float64)
    E = X[0].size
    Xp = np.repeat(X, E, axis=0).reshape(E, E)
    Xm = Xp.copy()
    Xp[np.arange(E), np.arange(E)] += eps
    Xm[np.arange(E), np.arange(E)] -= eps
    both = np.concatenate([Xp, Xm]).reshape((2 * E,) + X.shape[1:])
    K = gram(both, Y, kind, h, n).sum(axis=1)
    return ((K[:E] - K[E:]) / (2 * eps)).reshape(X.shape)
