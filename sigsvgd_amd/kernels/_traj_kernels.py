"""Trajectory kernels: `BatchGaussianKernel` (static RBF on path points; `BatchIMQKernel` and
`BatchRationalQuadraticKernel` are its heavy-tailed siblings, `BatchMatern32Kernel` and `BatchMatern52Kernel` its rougher
ones) and `SignatureKernel` (signature
kernel via the Goursat PDE) -- reference src/kernels/_traj_kernels.py:147-206 -- backed by the HIP library
instead of `sigkernel`; `PathSigKernel` (static kernel on truncated signatures, :72-144) backed by the HIP
signature kernel instead of `signatory`; `TrajectoryKernel` (:14-69)."""
from __future__ import annotations

import torch

from .. import _lib
from ..sigkernel import SigKernel, batch_sqdist, gram_sqdist, inv_bandwidth_from_fn, matern_radial, radial_power
from ._kernels import BaseKernel, GaussianKernel, _SqDist, kernel_output, scalar_function

class TrajectoryKernel(BaseKernel):
    """RBF kernel between state-space projections phi(actions) of the inputs; the gradient w.r.t. the
    actions comes from autograd through the caller's rollout graph (reference _traj_kernels.py:14-69).
    The pairwise distance is a HIP autograd node (`_SqDist`)."""

    def __init__(self, bandwidth_fn: scalar_function = None, **kwargs):
        super().__init__(bandwidth_fn, analytic_grad=False, **kwargs)

    def __call__(self, X, Y, X_actions, h: float = None, compute_grad=True, **kwargs) -> kernel_output:
        assert X.shape == Y.shape, "X and Y must have the same dimensions."
        sq_dists = _SqDist.apply(torch.atleast_2d(X), torch.atleast_2d(Y), None)
        h = self.get_bandwidth(sq_dists) if h is None else float(h)
        gamma = -0.5 / h**2
        K = (gamma * sq_dists).exp()
        if compute_grad:
            d_K = torch.autograd.grad(K.sum(), X_actions, retain_graph=True)[0]
            return K, d_K
        return K


class PathSigKernel(BaseKernel):
    """Static kernel on truncated path signatures S(X, depth) with a zero base point (reference
    _traj_kernels.py:72-144).  As in the reference, `h` and `ref_vector` are accepted but NOT forwarded:
    the static kernel uses its own bandwidth function, and the returned gradient is the static kernel's
    `d_K.sum(1)` with respect to the SIGNATURE features ([batch, C + ... + C^depth])."""

    def __init__(self, bandwidth_fn: scalar_function = None, static_kernel: BaseKernel = None, **kwargs):
        super().__init__(bandwidth_fn, analytic_grad=False, **kwargs)
        self.static_kernel = GaussianKernel() if static_kernel is None else static_kernel

    def __call__(self, X, Y, ref_vector=None, depth: int = 3, h: float = None, compute_grad=True,
                 **kwargs) -> kernel_output:
        from .. import ops

        assert X.shape == Y.shape, "X and Y must have the same dimensions."
        X, Y = torch.atleast_3d(X), torch.atleast_3d(Y)
        X_sig = ops.signature(X, depth, basepoint=True)
        Y_sig = ops.signature(Y, depth, basepoint=True)
        if compute_grad:
            K, d_K = self.static_kernel(X_sig, Y_sig, compute_grad=True)
            return K, d_K
        return self.static_kernel(X_sig, Y_sig, compute_grad=False)


class BatchGaussianKernel(BaseKernel):
    """RBF kernel on path points, k(x, y) = exp(-|x-y|^2 / h), h = bandwidth_fn(dist)."""

    static_kind = _lib.STATIC_RBF

    def __init__(self, bandwidth_fn: scalar_function = None, **kwargs):
        super().__init__(bandwidth_fn, analytic_grad=False, **kwargs)

    def __call__(self, X: torch.Tensor, Y: torch.Tensor, **kwargs) -> kernel_output:
        return self.batch_kernel(X, Y, **kwargs)

    def batch_kernel(self, X, Y, h=None):
        """X [batch, len_X, dim], Y [batch, len_Y, dim] -> k(X^i_s, Y^i_t) [batch, len_X, len_Y]."""
        A, M, N = X.shape[0], X.shape[1], Y.shape[1]
        Xs = torch.sum(X**2, dim=2)
        Ys = torch.sum(Y**2, dim=2)
        dist = -2.0 * torch.bmm(X, Y.permute(0, 2, 1))
        dist += torch.reshape(Xs, (A, M, 1)) + torch.reshape(Ys, (A, 1, N))
        h = self.get_bandwidth(dist) if h is None else float(h)
        return torch.exp(-dist / h)

    def Gram_matrix(self, X, Y, h=None):
        """X [A, len_X, dim], Y [B, len_Y, dim] -> k(X^i_s, Y^j_t) [A, B, len_X, len_Y]."""
        dist = gram_sqdist(X, Y)
        h = self.get_bandwidth(dist) if h is None else float(h)
        return torch.exp(-dist / h)

    def inv_bandwidth(self, X, Y) -> float:
        """1/h for the fused HIP path (constant bandwidth functions never form the distance tensor)."""
        return inv_bandwidth_from_fn(self.get_bandwidth, X, Y)


class BatchIMQKernel(BaseKernel):
    """Inverse multiquadric on path points, k(x, y) = (1 + |x-y|^2 / h)^(-1/2), h = bandwidth_fn(dist): heavy-tailed where
    the RBF kernel underflows.  Bandwidths resolve as BatchGaussianKernel's do (`inv_bandwidth_from_fn`: constant functions
    form no distances, the default median comes from the select on the device)."""

    static_kind = _lib.STATIC_IMQ
    power = -0.5

    def __init__(self, bandwidth_fn: scalar_function = None, **kwargs):
        super().__init__(bandwidth_fn, analytic_grad=False, **kwargs)

    def __call__(self, X: torch.Tensor, Y: torch.Tensor, **kwargs) -> kernel_output:
        return self.batch_kernel(X, Y, **kwargs)

    def _of(self, dist, h):
        return radial_power(dist, self.get_bandwidth(dist) if h is None else float(h), self.power)

    def batch_kernel(self, X, Y, h=None):
        """X [batch, len_X, dim], Y [batch, len_Y, dim] -> k(X^i_s, Y^i_t) [batch, len_X, len_Y]."""
        return self._of(batch_sqdist(X, Y), h)

    def Gram_matrix(self, X, Y, h=None):
        """X [A, len_X, dim], Y [B, len_Y, dim] -> k(X^i_s, Y^j_t) [A, B, len_X, len_Y]."""
        return self._of(gram_sqdist(X, Y), h)

    def inv_bandwidth(self, X, Y) -> float:
        """1/h for the fused HIP path (constant bandwidth functions never form the distance tensor)."""
        return inv_bandwidth_from_fn(self.get_bandwidth, X, Y)


class BatchRationalQuadraticKernel(BatchIMQKernel):
    """Rational quadratic kernel on path points, k(x, y) = (1 + |x-y|^2 / h)^(-1), h = bandwidth_fn(dist)."""

    static_kind = _lib.STATIC_RQ
    power = -1.0


class BatchMatern32Kernel(BatchIMQKernel):
    """Matern-3/2 kernel on path points, k = (1 + u) exp(-u), u = sqrt(3 |x-y|^2 / h), h = bandwidth_fn(dist): a Matern kernel
    of lengthscale l is h = l^2.  Bandwidths resolve as BatchGaussianKernel's do."""

    static_kind = _lib.STATIC_MATERN32
    power = None  # (not a power of 1 + dist / h)
    order = 3

    def _of(self, dist, h):
        return matern_radial(dist, self.get_bandwidth(dist) if h is None else float(h), self.order)


class BatchMatern52Kernel(BatchMatern32Kernel):
    """Matern-5/2 kernel on path points, k = (1 + u + u^2 / 3) exp(-u), u = sqrt(5 |x-y|^2 / h), h = bandwidth_fn(dist)."""

    static_kind = _lib.STATIC_MATERN52
    order = 5


_STATIC_BY_NAME = {"rbf": BatchGaussianKernel, "imq": BatchIMQKernel, "rq": BatchRationalQuadraticKernel,
                   "matern32": BatchMatern32Kernel, "matern52": BatchMatern52Kernel}


class SignatureKernel:
    """Signature kernel with a static kernel on path points; `depth` is the DYADIC ORDER of the PDE solver
    (not a truncation level).  static_kernel: None or "rbf" (the reference's RBF), "imq", "rq", "matern32", "matern52" (each built on
    `bandwidth_fn`), or a static-kernel instance, used as it is.  fp32_sweeps: `SigKernel`'s (the IMQ and rational-quadratic kernels,
    and RBF paths of 17 to 32 channels, on the register-resident fp32-sweep kernel at order 0, T <= 64).  exact_grad: `SigKernel`'s (every gradient the exact derivative of
    the discrete kernel, on the long route).  normalize: `SigKernel`'s (the normalised kernel
    K(x, y) / sqrt(K(x, x) K(y, y)) from the long route's log-domain launches: `__call__` through `compute_Gram`, `gram_and_grad` --
    and with it `SVGD` and `ScoreEstimator` -- from one launch with SIGSVGD_FLAG_NORMALIZED).
    normalize_route: `SigKernel`'s ("fused": the normalised kernel around the fused Gram launch, one
    `ops.gram_fwd_bwd(..., normalized=True)` per `gram_and_grad`).  Unknown
    keyword arguments are accepted and ignored, as in
    the reference (examples/script_planning_robot.py:391 passes `bandwidth=`)."""

    def __init__(self, bandwidth_fn: scalar_function = None, depth: int = 3, static_kernel=None, fp32_sweeps: bool = False,
                 exact_grad: bool = False, normalize: bool = False, normalize_route: str = "long", **kwargs):
        if static_kernel is None or isinstance(static_kernel, str):
            name = "rbf" if static_kernel is None else static_kernel.lower()
            if name not in _STATIC_BY_NAME:
                raise ValueError(f'static_kernel must be one of {sorted(_STATIC_BY_NAME)} or an instance, got {static_kernel!r}')
            static_kernel = _STATIC_BY_NAME[name](bandwidth_fn=bandwidth_fn)
        self.kernel = SigKernel(static_kernel, dyadic_order=depth, fp32_sweeps=fp32_sweeps, exact_grad=exact_grad,
                                normalize=normalize, normalize_route=normalize_route)

    def __call__(self, X, Y, **kwargs):
        # The reference upcasts to fp64 around compute_Gram and casts K back; the HIP kernels read fp32/fp64 paths
        # directly (static kernel and increments in fp64, sweeps in fp32 difference form or fp64 depending on the
        # kernel: DESIGN.md §3), so no copies are needed.
        return self.kernel.compute_Gram(X, Y)

    def gram_and_grad(self, X, grad_out=None):
        """(K, grad_k) in one fused launch == `K = self(X, X.detach()); ag(K.sum(), X)`."""
        return self.kernel.gram_and_grad(X, None, grad_out)
