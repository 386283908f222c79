"""Shared inputs and error metrics of the parity tests: the seeded path generators, the two metrics of the accuracy
contract, and the small doubles (a static kernel the library cannot recognise, a cost function) several files use.
tests/test_support.py pins the generators to literal values and the metrics to hand-computed ones."""
import numpy as np
import torch


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def walks(A, T, d, seed, scale, offset=0.0):
    """[A, T, d] fp32 random walks from `seed`: cumulative sums of steps `scale` * N(0, 1), shifted by `offset`.  `scale` sets
    the regime and has no default: 0.05 is the smooth one of the order-0 parity files, 0.3 that of the refined grids."""
    rng = np.random.default_rng(seed)
    return (np.cumsum(scale * rng.standard_normal((A, T, d)), axis=1) + offset).astype(np.float32)


def sized_walks(rng, B, T, d, scale=1.0):
    """[B, T, d] fp32 random walks drawn from `rng`, of about `scale` overall size whatever their length"""
    return np.cumsum(scale / np.sqrt(T) * rng.standard_normal((B, T, d)), axis=1).astype(np.float32)


def bounded_points(seed, A, T, d, sd):
    """[A, T, d] fp32 paths of independent points `sd` * N(0, 1) from `seed`: bounded, so a static kernel of bandwidth 1 never
    decays along the path, and rough, so the signature kernel still grows (tests/long_reference.py)"""
    return (sd * np.random.default_rng(seed).standard_normal((A, T, d))).astype(np.float32)


def signed_weights(A, B, seed):
    """grad_out with every entry of the same order and random sign: w = s u, s = +-1, u uniform in [0.5, 1.5] -- no pair
    is hidden behind a weight near zero"""
    rng = np.random.default_rng(seed)
    return rng.choice([-1.0, 1.0], size=(A, B)) * rng.uniform(0.5, 1.5, size=(A, B))


def np64(t):
    return t.detach().double().cpu().numpy()


def _f64(a):
    return np64(a) if hasattr(a, "detach") else np.asarray(a, np.float64)


# ---- metrics --------------------------------------------------------------------------------------------------------------
def rel_max(a, b, zero_ok=False):
    """max|a - b| / max|b| of tensors or arrays: the metric of gradients, phi and updates, whose entries pass through zero.
    An all-zero reference says nothing about `a` and fails; `zero_ok=True` is for the call site that means to compare with
    exact zeros (the result is then 0 where `a` is zero too, and huge otherwise)."""
    a, b = _f64(a), _f64(b)
    top = np.abs(b).max()
    assert zero_ok or top > 0, "rel_max: the reference is all zero (or not finite)"
    return float(np.abs(a - b).max() / max(top, 1e-300))


def rel_entry(K, K_ref, floor, min_ref=None):
    """max over entries of |K - K_ref| / max(|K_ref|, floor): the per-entry contract of the Gram matrix (K > 0 always).
    The floors in use:
      1e-6  plain relative error per entry; the floor only keeps an exact zero out of the denominator.  The contract of
            the fp32-sweep kernels since pairs whose K is small against their grid go through the exact fp64 pass
            (DESIGN.md section 3).
      0     the same without the guard: the fp64 long-path, paired and static-kind files, whose references stay away from
            zero (`min_ref` asserts that: the smallest |K_ref| allowed).
      0.1   the earlier contract, which lets entries below 0.1 off with an absolute 0.1 * tol: tests/test_gpu_pde.py only,
            kept as that file has it."""
    K, K_ref = _f64(K), _f64(K_ref)
    if min_ref is not None:
        assert np.abs(K_ref).min() >= min_ref, np.abs(K_ref).min()
    return float((np.abs(K - K_ref) / np.maximum(np.abs(K_ref), floor)).max())


# ---- doubles --------------------------------------------------------------------------------------------------------------
class DisguisedRBF:
    """exp(-|x - y|^2 / sigma) behind upstream's interface only: the library cannot recognise it (user route)."""

    def __init__(self, sigma):
        self.sigma = sigma

    def Gram_matrix(self, X, Y):
        dist = (X**2).sum(-1)[:, None, :, None] + (Y**2).sum(-1)[None, :, None, :] - 2.0 * torch.einsum("ipk,jqk->ijpq", X, Y)
        return torch.exp(-dist / self.sigma)

    def batch_kernel(self, X, Y):
        dist = (X**2).sum(-1)[:, :, None] + (Y**2).sum(-1)[:, None, :] - 2.0 * torch.bmm(X, Y.transpose(1, 2))
        return torch.exp(-dist / self.sigma)


def gram_and_xgrad(kernel, X, Y, W, sym):
    """(K, d sum(W K) / dX) through `kernel.compute_Gram` and autograd; W None: uniform weights"""
    Xg = X.detach().clone().requires_grad_(True)
    K = kernel.compute_Gram(Xg, Xg if sym else Y, sym=sym)
    loss = K.sum() if W is None else (K * W).sum()
    (gX,) = torch.autograd.grad(loss, Xg)
    return K.detach(), gX


def path_cost_fn(x, w):
    c = w * (x**2).sum((1, 2)) + ((x[:, 1:] - x[:, :-1]) ** 2).sum((1, 2))
    return c, {"aux": c.detach() * 2}
