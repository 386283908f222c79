"""fp64 numpy reference of the log-domain signature kernel (SIGSVGD_FLAG_LOG_K), shared by
tests/test_log_k_cpu.py and tests/test_gpu_log_k.py: ln K and the gradient of ln K in the GG convention, for pairs whose K
overflows fp64.

Both Goursat sweeps are linear in the solution, so the solution may be carried times any positive factor.  Here every
anti-diagonal of the refined grid is divided by a factor of its own (by default its largest entry; `factor` gives any other,
and the results do not depend on it beyond rounding) and the logarithms of the factors are summed:

    K[p][q] = Ks[p][q] exp(c[p + q]),         K_rev[p][q] = Rs[p][q] exp(e[p + q]),
    ln K = ln Ks[P][Q] + c[P + Q],
    GG[p][q] / K = Ks[p][q] Rs[p+1][q+1] exp(c[p + q] + e[p + q + 2] - ln K),

and S = dK/dD / K is the block sum of GG / K over r^2.  (The kernels rescale by powers of two between blocks of 64 sweep steps,
a band at a time; the restatement is independent of that on purpose.)  Everything behind S is tests/exact_adjoint_reference.py's:
the 4-corner scatter and the static kernels' own derivatives.  A pair whose discrete K is <= 0 gives NaN."""
import numpy as np

import exact_adjoint_reference as EA
from oracle import sigkernel_oracle as O

RBF, LINEAR, IMQ, RQ, MATERN32, MATERN52 = EA.KINDS


def _by_max(s, v):
    return np.abs(v).max(axis=-1)


def scaled_sweep(g, factor=_by_max, dtype=np.float64):
    """increments g [..., P, Q] -> (Ks [..., P+1, Q+1], c [..., P+Q+1]) with K[p][q] = Ks[p][q] exp(c[p+q]); factor(s, v) > 0
    [...]: what anti-diagonal s (values v [..., cells]) is divided by"""
    g = np.asarray(g, dtype=dtype)
    P, Q = g.shape[-2:]
    lead = g.shape[:-2]
    Ks = np.ones(lead + (P + 1, Q + 1), dtype=dtype)
    c = np.zeros(lead + (P + Q + 1,), dtype=dtype)
    for s in range(P + Q - 1):  # the cells (p+1, q+1) with p + q = s from the anti-diagonals s + 1 and s of K
        p = np.arange(max(0, s - Q + 1), min(P, s + 1))
        q = s - p
        gg = g[..., p, q]
        g2 = gg * gg / 12
        # bring the two anti-diagonals read to the scale of the newer one
        down = np.exp(c[..., s] - c[..., s + 1])[..., None]
        new = (Ks[..., p + 1, q] + Ks[..., p, q + 1]) * (1 + gg / 2 + g2) - Ks[..., p, q] * down * (1 - g2)
        # the anti-diagonal s + 2: the new cells and its two edge cells, K = 1, at the running scale
        edge = np.exp(-c[..., s + 1])
        if s + 2 <= Q:
            Ks[..., 0, s + 2] = edge
        if s + 2 <= P:
            Ks[..., s + 2, 0] = edge
        f = np.asarray(factor(s, new), dtype=dtype)
        Ks[..., p + 1, q + 1] = new / f[..., None]
        if s + 2 <= Q:
            Ks[..., 0, s + 2] /= f
        if s + 2 <= P:
            Ks[..., s + 2, 0] /= f
        c[..., s + 2] = c[..., s + 1] + np.log(f)
    return Ks, c


def log_pde(G, n=0, factor=_by_max):
    """static-kernel grids G [..., M, N] -> (ln K [...], S [..., M-1, N-1] = dK/dD / K, R [..., M, N] = dK/dG / K)"""
    g = O.refine(O.increments(np.asarray(G, dtype=np.float64)), n)
    P, Q = g.shape[-2:]
    Ks, c = scaled_sweep(g, factor)
    Rs, e = scaled_sweep(g[..., ::-1, ::-1], factor)
    Rs = Rs[..., ::-1, ::-1]  # K_rev[p][q] = Rs[p][q] exp(e[P + Q - p - q])
    m = Ks[..., P, Q]
    with np.errstate(invalid="ignore", divide="ignore"):
        lnK = np.where(m > 0, np.log(np.where(m > 0, m, 1.0)) + c[..., P + Q], np.nan)
    s = np.add.outer(np.arange(P), np.arange(Q))  # p + q
    expo = c[..., s] + e[..., (P + Q - 2) - s] - lnK[..., None, None]
    S = EA.block_sum(Ks[..., :-1, :-1] * Rs[..., 1:, 1:] * np.exp(expo), n)
    return lnK, S, EA.scatter(S)


def _chain(X, Y, wR, kind, h):
    """(gX [A,TX,d], gY [B,TY,d]) from weighted dK/dG [A,B,TX,TY]: exact_adjoint_reference.gram_backward's last step"""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    if kind == LINEAR:
        return np.einsum("ijmn,jnc->imc", wR, Y), np.einsum("ijmn,imc->jnc", wR, X)
    diff = EA._diff(X, Y)
    s = (diff * diff).sum(-1) / float(h)
    core = (wR * EA._profile(kind).neg_dphi(kind, s))[..., None] * diff * (2.0 / float(h))
    return -core.sum(axis=(1, 3)), core.sum(axis=(0, 2))


def log_gram(X, Y, kind=RBF, h=1.0, n=0, factor=_by_max):
    return log_pde(EA.static_gram(X, Y, kind, h), n, factor)[0]


def cancellation(X, Y, kind=RBF, h=1.0, n=0):
    """[A, B] >= 1: the largest |K[p][q]| on a pair's grid over its final K.  Every step of a sweep rounds relative to the
    values it adds, so a pair whose K is what is left of larger terms carries their rounding: an fp64 sweep knows its ln K to
    about this factor times what it knows a K that grew monotonically to."""
    g = O.refine(O.increments(EA.static_gram(X, Y, kind, h)), n)
    P, Q = g.shape[-2:]
    Ks, c = scaled_sweep(g)
    with np.errstate(divide="ignore"):
        size = np.log(np.abs(Ks)) + c[..., np.add.outer(np.arange(P + 1), np.arange(Q + 1))]
    return np.exp(size.max(axis=(-2, -1)) - size[..., P, Q])


def log_gram_backward(X, Y, w=None, kind=RBF, h=1.0, n=0, sym=False, factor=_by_max):
    """-> (ln K [A,B], gX [A,TX,d], gY [B,TY,d]): the gradients of sum(w ln K) (w ones when None; sym: w + w^T)"""
    lnK, _, R = log_pde(EA.static_gram(X, Y, kind, h), n, factor)
    w = np.ones(lnK.shape) if w is None else np.asarray(w, dtype=np.float64)
    if sym:
        w = w + w.T
    return (lnK, *_chain(X, Y, w[:, :, None, None] * R, kind, h))


def log_pair_backward(X, Y, w=None, kind=RBF, h=1.0, n=0, factor=_by_max):
    """-> (ln K [A], gX [A,TX,d], gY [A,TY,d]) of the pairs (X_i, Y_i), weights w [A]"""
    A = len(X)
    w = np.ones(A) if w is None else np.asarray(w, dtype=np.float64)
    out = [log_gram_backward(X[i:i + 1], Y[i:i + 1], w[i].reshape(1, 1), kind, h, n, False, factor) for i in range(A)]
    return (np.array([o[0][0, 0] for o in out]), np.concatenate([o[1] for o in out]), np.concatenate([o[2] for o in out]))


def longdouble_log_K(G, n=0):
    """ln K of ONE grid G [M, N] from the plain, unscaled sweep in np.longdouble (x87: finite up to 1e4932)"""
    g = O.refine(O.increments(np.asarray(G, dtype=np.longdouble)), n)
    P, Q = g.shape
    K = np.ones((P + 1, Q + 1), dtype=np.longdouble)
    for s in range(P + Q - 1):
        p = np.arange(max(0, s - Q + 1), min(P, s + 1))
        q = s - p
        gg = g[p, q]
        g2 = gg * gg / 12
        K[p + 1, q + 1] = (K[p + 1, q] + K[p, q + 1]) * (1 + gg / 2 + g2) - K[p, q] * (1 - g2)
    return np.log(K[-1, -1])


def walks(seed, A, T, d, step, dtype=np.float64):
    """Gaussian random walks [A, T, d] with steps of standard deviation `step` per channel"""
    rng = np.random.default_rng(seed)
    return np.cumsum(step * rng.standard_normal((A, T, d)), axis=1).astype(dtype)


# ---- the normalised kernel built from ln K and its gradients (the composition of sigsvgd_amd.sigkernel, section 5.21) -------------
def normalized_gram_and_grads(X, Y, G_up, kind=RBF, h=1.0, n=0, same=False):
    """-> (Khat [A,B], gX, gY): Khat_ij = exp(l_ij - a_i / 2 - b_j / 2) and the gradients of sum(G_up Khat) in X and Y (each
    tensor's own; same: X is Y, one gradient, the sum), built from this module's ln K and gradients of ln K alone"""
    l = log_gram(X, Y, kind, h, n)
    a = log_pair_backward(X, X, None, kind, h, n)[0]
    b = a if same else log_pair_backward(Y, Y, None, kind, h, n)[0]
    Khat = np.exp(l - 0.5 * a[:, None] - 0.5 * b[None, :])
    W = np.asarray(G_up, np.float64) * Khat
    _, gX, gY = log_gram_backward(X, Y, W, kind, h, n)
    _, ax, ay = log_pair_backward(X, X, -0.5 * W.sum(1), kind, h, n)
    _, bx, by = log_pair_backward(Y, Y, -0.5 * W.sum(0), kind, h, n)
    gX, gY = gX + ax + ay, gY + bx + by
    return (Khat, gX + gY, None) if same else (Khat, gX, gY)


def torch_K(X, Y, h=1.0):
    """K [A, B] of the RBF static kernel at order 0 as a torch autograd node on fp64 CPU tensors: the oracle's K forward, the
    oracle's gradients backward (the GG convention of the library, each slot its own; shapes whose K stays inside fp64)"""
    import torch

    class OracleGram(torch.autograd.Function):
        @staticmethod
        def forward(ctx, X, Y):
            ctx.save_for_backward(X, Y)
            return torch.as_tensor(O.gram(X.numpy(), Y.numpy(), O.RBF, h, 0))

        @staticmethod
        def backward(ctx, G):
            X, Y = (t.numpy() for t in ctx.saved_tensors)
            return (torch.as_tensor(O.gram_backward(X, Y, G.numpy(), O.RBF, h, 0)[1]),
                    torch.as_tensor(O.gram_backward(Y, X, G.numpy().T, O.RBF, h, 0)[1]))

    return OracleGram.apply(X, Y)


def normalized_torch(X, Y, h=1.0):
    """K(X_i, Y_j) / sqrt(K(X_i, X_i) K(Y_j, Y_j)) from torch_K: torch autograd does the algebra of the normalisation"""
    import torch

    return torch_K(X, Y, h) / torch.sqrt(torch_K(X, X, h).diagonal()[:, None] * torch_K(Y, Y, h).diagonal()[None, :])
