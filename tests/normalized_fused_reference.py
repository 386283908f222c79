"""fp64 numpy restatement of the fused route's normalised launch (SIGSVGD_FLAG_NORMALIZED_FUSED),
shared by tests/test_normalized_fused_cpu.py and tests/test_gpu_normalized_fused.py.

`gram_and_grad` states the pipeline's algebra on the plain oracle (oracle/sigkernel_oracle.py: the unscaled K and its
first-slot GG gradient; the RBF and linear kinds, which that oracle has):

    a_i = ln K(X_i, X_i),  b_j = ln K(Y_j, Y_j),  s_ij = exp(-(a_i + b_j) / 2),  K^_ij = K_ij s_ij,
    W'_ij = w_ij s_ij                    (SYM: (w_ij + w_ji) s_ij; Y_IS_X: 0 on the diagonal)
    t1_i  = sum_j W'_ij d1 K_ij          the unflagged launch's gradient under the weights W'
    U_i   = sum_j w_ij K^_ij             (the same w; Y_IS_X: without the diagonal)
    t2_i  = 1/2 U_i grad a_i             grad a_i = (d1 + d2) K(X_i, X_i) / K(X_i, X_i) = 2 d1 K(X_i, X_i) / K(X_i, X_i)
    gradX_i = t1_i - t2_i

(K is symmetric in its two paths and so is GG on the grid of a pair (x, x): the second-slot gradient of K(x, x) equals the
first-slot one.)  tests/test_normalized_fused_cpu.py holds this to 1e-10 of the largest entry against the yardstick of the
GPU tests, `log_k_reference.normalized_gram_and_grads`, which is built from logarithms alone.  `terms` returns the same two
terms for every static kind, from that module's pieces: the GPU tests' bound is 1e-5 (max|t1| + max|t2|)."""
import numpy as np

import log_k_reference as R
from oracle import sigkernel_oracle as O


def _weights(w, A, B, sym, y_is_x):
    w = np.ones((A, B)) if w is None else np.asarray(w, dtype=np.float64)
    if sym:
        w = w + w.T
    if y_is_x:
        w = w - np.diag(np.diag(w))
    return w


def gram_and_grad(X, Y, w=None, kind=O.RBF, h=1.0, n=0, sym=False, y_is_x=False):
    """-> (K^ [A,B], gradX [A,T,d], t1, t2) of the launch with grad_out = w (None: ones); y_is_x: Y is X's values"""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    A, B = len(X), len(Y)
    diag = [O.gram_backward(X[i:i + 1], X[i:i + 1], None, kind, h, n) for i in range(A)]
    Kxx = np.array([k[0, 0] for k, _ in diag])
    grad_a = np.concatenate([2.0 * g / k[0, 0] for k, g in diag])
    Kyy = Kxx if y_is_x else np.array([O.gram(Y[j:j + 1], Y[j:j + 1], kind, h, n)[0, 0] for j in range(B)])
    s = np.exp(-0.5 * (np.log(Kxx)[:, None] + np.log(Kyy)[None, :]))
    w = _weights(w, A, B, sym, y_is_x)
    K, t1 = O.gram_backward(X, Y, w * s, kind, h, n)
    Khat = K * s
    if y_is_x:
        np.fill_diagonal(Khat, 1.0)
    t2 = 0.5 * (w * Khat).sum(1)[:, None, None] * grad_a
    return Khat, t1 - t2, t1, t2


def terms(X, Y, w=None, kind=R.RBF, h=1.0, n=0, sym=False, y_is_x=False):
    """-> (t1, t2) as above for any static kind, from log_k_reference: t1 = sum_j U_ij d1 ln K_ij (U_ij K_ij^-1 = W'_ij),
    t2 = 1/2 (sum_j U_ij) grad ln K(X_i, X_i)"""
    l = R.log_gram(X, Y, kind, h, n)
    a = R.log_pair_backward(X, X, None, kind, h, n)[0]
    b = a if y_is_x else R.log_pair_backward(Y, Y, None, kind, h, n)[0]
    U = _weights(w, len(X), len(Y), sym, y_is_x) * np.exp(l - 0.5 * a[:, None] - 0.5 * b[None, :])
    t1 = R.log_gram_backward(X, Y, U, kind, h, n)[1]
    _, ax, ay = R.log_pair_backward(X, X, 0.5 * U.sum(1), kind, h, n)
    return t1, ax + ay
