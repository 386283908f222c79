"""`sigkernel`-compatible front end of the HIP signature-kernel path.

The reference delegates the Goursat-PDE arithmetic to the third-party package `sigkernel`
(/root/reference/setup.py:71) and uses exactly this surface of it:

    sigkernel.SigKernel(static_kernel, dyadic_order)            src/kernels/_traj_kernels.py:201
        .compute_Gram(X.double(), Y.double(), sym=False)        src/kernels/_traj_kernels.py:205,
                                                                src/inference/trajectory_svgd.py:60-62
    sigkernel.RBFKernel(sigma)                                  examples/script_control_particle_maze.py:43
    isinstance(kernel, sigkernel.SigKernel)                     src/inference/trajectory_svgd.py:55

This module provides those names on top of libsigsvgd_hip.so, so `sys.modules["sigkernel"] =
sigsvgd_amd.sigkernel` makes the reference's own code run on the MI355X path.
`compute_Gram` is an autograd node: backward receives grad_output [A,B] and returns the gradient
for X only (None for everything else), like upstream; `grad_Y=True` adds the second-slot gradient for Y.  `compute_kernel` (and `compute_distance` on it) solves each pair
(X_i, Y_i) once and differentiates both paths, each in its own slot.

Static kernels.  `RBFKernel`, `LinearKernel`, the heavy-tailed `IMQStaticKernel` and `RationalQuadraticKernel`, the rougher
`Matern32StaticKernel` and `Matern52StaticKernel`, anything with
`static_kind` + `inv_bandwidth` (`sigsvgd_amd.kernels.BatchGaussianKernel`, `BatchIMQKernel`, `BatchRationalQuadraticKernel`,
`BatchMatern32Kernel`, `BatchMatern52Kernel`)
and the reference's own `BatchGaussianKernel` are evaluated inside the fused HIP kernels (nothing of size [A,B,T,T] is formed); paths too long for
the fused kernels' LDS take the long route (csrc/gram_long.hip), which evaluates the static kernel inside its PDE sweep
(P, Q <= 8192 refined cells).  RBF alone has the fp32-sweep kernels; the linear, IMQ, rational-quadratic and Matern kernels run
on the fp64 coverage kernel and the long route (there, but for the linear kernel, with the default stencil only: DESIGN.md
sections 5.15, 5.17).  A `BatchGaussianKernel` without a `bandwidth_fn` (the reference's default, the median
heuristic) takes its median from an exact select on the device (`ops.path_sqdist_select`), at any batch size.  Any other object with upstream's `Gram_matrix(X, Y) -> [A,B,M,N]` (and, optionally,
`batch_kernel(X, Y) -> [A,M,N]`) is a USER static kernel: its grid is materialised by the user's own torch code, as upstream does, and the signature PDE on it runs on
the device (`ops.PDESolve`, csrc/sig_pde.hip).  Gradients then flow through torch autograd -- to X through the user's
`Gram_matrix` and to the static kernel's own parameters.  The grid costs A*B*M*N elements of memory: large batches
belong on the built-in kernels.  Objects without `Gram_matrix` raise NotImplementedError.

Learning sigma.  Where the `sigma` of `RBFKernel`, `IMQStaticKernel`, `RationalQuadraticKernel`,
`Matern32StaticKernel` or `Matern52StaticKernel` is a one-element tensor that requires grad (on any device) and grad mode is on, `compute_Gram` and `compute_kernel` -- and
`compute_distance` / `compute_mmd` through them -- are autograd nodes that take sigma as an input: they run on the long route's
bandwidth launches (`ops.gram_long_fwd_bwd_h`, `ops.pair_fwd_bwd_h`) whatever the shape, save every pair's dK/d(1/sigma) in
forward and return grad_sigma = -(1/sigma)^2 sum(grad_output * dK/d(1/sigma)) without another launch, in the reference's GG
convention (what upstream's autograd through its torch static kernels gives).  X and Y keep the rules above.  Shapes the long
route refuses, and IMQ / rational quadratic / Matern with `_naive_solver=True`, raise NotImplementedError.  A float sigma, a tensor
that does not require grad and `torch.no_grad()` take exactly the launches described above.  Data-dependent bandwidths (the
median) stay detached, as in the reference.

Paths of different lengths in one batch.  `compute_Gram`, `compute_kernel`, `compute_distance` and
`compute_mmd` take `lengths_X` / `lengths_Y` ([A] / [B] integers in [1, T], a tensor on either device or a sequence): path i is
its first `lengths_X[i]` points, whatever the rest of its row holds.  The layer replaces the rest by NaN on the device (no
sync; the padded entries get a zero gradient) and sends every request, forward or gradient, to the long route's launches with
SIGSVGD_FLAG_NAN_TAILS (`ops.gram_long_fwd_bwd2`, `ops.pair_fwd*` with `nan_tails=True`), which solve every pair on its own
grid.  Built-in static kernels with an explicit bandwidth only; see `SigKernel.compute_Gram`.  Without lengths every call
reaches `ops` exactly as described above.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib, ops

__all__ = ["SigKernel", "RBFKernel", "LinearKernel", "IMQStaticKernel", "RationalQuadraticKernel", "Matern32StaticKernel",
           "Matern52StaticKernel", "gram_and_grad"]


# ------------------------------------------------------------------------------------------------
# static kernels
# ------------------------------------------------------------------------------------------------
class LinearKernel:
    """k(x, y) = <x, y>."""

    static_kind = _lib.STATIC_LINEAR

    def inv_bandwidth(self, X, Y) -> float:
        return 1.0

    def batch_kernel(self, X, Y):
        return torch.bmm(X, Y.permute(0, 2, 1))

    def Gram_matrix(self, X, Y):
        return torch.einsum("ipk,jqk->ijpq", X, Y)


def _sigma_value(sigma) -> float:
    """sigma as a float; a tensor (also one that requires grad: SigKernel differentiates it) is read
    detached"""
    return float(sigma.detach()) if isinstance(sigma, torch.Tensor) else float(sigma)


class RBFKernel:
    """k(x, y) = exp(-|x-y|^2 / sigma)   (sigkernel's convention: divide by sigma, not 2 sigma^2)."""

    static_kind = _lib.STATIC_RBF

    def __init__(self, sigma):
        self.sigma = sigma

    def inv_bandwidth(self, X, Y) -> float:
        return 1.0 / _sigma_value(self.sigma)

    def batch_kernel(self, X, Y):
        Xs = torch.sum(X**2, dim=2)
        Ys = torch.sum(Y**2, dim=2)
        dist = -2.0 * torch.bmm(X, Y.permute(0, 2, 1))
        dist = dist + Xs[:, :, None] + Ys[:, None, :]
        return torch.exp(-dist / self.sigma)

    def Gram_matrix(self, X, Y):
        Xs = torch.sum(X**2, dim=2)
        Ys = torch.sum(Y**2, dim=2)
        dist = -2.0 * torch.einsum("ipk,jqk->ijpq", X, Y)
        dist = dist + Xs[:, None, :, None] + Ys[None, :, None, :]
        return torch.exp(-dist / self.sigma)


def batch_sqdist(X, Y):
    """dist[i,p,q] = |X_ip - Y_iq|^2 of paired batches X [A,M,d], Y [A,N,d]"""
    Xs = torch.sum(X**2, dim=2)
    Ys = torch.sum(Y**2, dim=2)
    dist = -2.0 * torch.bmm(X, Y.permute(0, 2, 1))
    return dist + Xs[:, :, None] + Ys[:, None, :]


def radial_power(dist, h, power):
    """(1 + dist / h)^power: the IMQ (power -1/2) and rational-quadratic (power -1) kernels of a squared distance"""
    return (1.0 + dist / h) ** power


class IMQStaticKernel:
    """k(x, y) = (1 + |x-y|^2 / sigma)^(-1/2): the inverse multiquadric, whose tail decays like 1/|x-y| where RBF's
    underflows (distant paths keep a non-zero signature-kernel gradient)."""

    static_kind = _lib.STATIC_IMQ
    power = -0.5

    def __init__(self, sigma):
        self.sigma = sigma

    def inv_bandwidth(self, X, Y) -> float:
        return 1.0 / _sigma_value(self.sigma)

    def batch_kernel(self, X, Y):
        return radial_power(batch_sqdist(X, Y), self.sigma, self.power)

    def Gram_matrix(self, X, Y):
        return radial_power(gram_sqdist(X, Y), self.sigma, self.power)


class RationalQuadraticKernel(IMQStaticKernel):
    """k(x, y) = (1 + |x-y|^2 / sigma)^(-1): the rational quadratic kernel of shape parameter 1."""

    static_kind = _lib.STATIC_RQ
    power = -1.0


def matern_radial(dist, h, order):
    """The Matern kernel of a squared distance: order 3 is (1 + u) e^-u with u = sqrt(3 dist / h), order 5 is
    (1 + u + u^2 / 3) e^-u with u = sqrt(5 dist / h).  dist / h is clamped at 0 (a distance formed from dot products can round
    below it), and the square root is taken where it is positive only, so autograd through coincident points gives the zero
    gradient term they have instead of sqrt's inf * 0."""
    s = dist / h
    pos = s > 0
    u = torch.where(pos, torch.sqrt(float(order) * torch.where(pos, s, torch.ones_like(s))), torch.zeros_like(s))
    poly = 1.0 + u if order == 3 else 1.0 + u + u * u / 3.0
    return poly * torch.exp(-u)


class Matern32StaticKernel:
    """k(x, y) = (1 + u) exp(-u), u = sqrt(3 |x-y|^2 / sigma): the Matern kernel of smoothness 3/2 (once differentiable sample
    paths).  sigma divides the squared distance, as RBFKernel's does: a lengthscale l is sigma = l^2."""

    static_kind = _lib.STATIC_MATERN32
    order = 3

    def __init__(self, sigma):
        self.sigma = sigma

    def inv_bandwidth(self, X, Y) -> float:
        return 1.0 / _sigma_value(self.sigma)

    def batch_kernel(self, X, Y):
        return matern_radial(batch_sqdist(X, Y), self.sigma, self.order)

    def Gram_matrix(self, X, Y):
        return matern_radial(gram_sqdist(X, Y), self.sigma, self.order)


class Matern52StaticKernel(Matern32StaticKernel):
    """k(x, y) = (1 + u + u^2 / 3) exp(-u), u = sqrt(5 |x-y|^2 / sigma): the Matern kernel of smoothness 5/2 (twice
    differentiable sample paths)."""

    static_kind = _lib.STATIC_MATERN52
    order = 5


# refuse to materialise distance tensors larger than this for data-dependent bandwidths
_MAX_DIST_BYTES = 4 << 30


class _ConstantProbe:
    """Stand-in handed to a `bandwidth_fn` first: constant lambdas (`lambda _: 0.03`, the norm in the
    reference's scripts, e.g. examples/script_planning_obstacle_field.py:321) return without touching
    it, so the [A,B,T,T] distance tensor never has to exist.  Any use of it raises."""

    class Touched(Exception):
        pass

    def _touch(self, *a, **k):
        raise _ConstantProbe.Touched()

    __getattr__ = _touch
    __add__ = __radd__ = __sub__ = __rsub__ = __mul__ = __rmul__ = __truediv__ = __rtruediv__ = _touch
    __neg__ = __pow__ = __getitem__ = __len__ = __iter__ = __float__ = __array__ = _touch
    __lt__ = __le__ = __gt__ = __ge__ = __bool__ = _touch

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        raise _ConstantProbe.Touched()


def gram_sqdist(X, Y):
    """dist[i,j,p,q] = |X_ip|^2 + |Y_jq|^2 - 2<X_ip,Y_jq> (reference _traj_kernels.py:186-190)."""
    A, B, M, N = X.shape[0], Y.shape[0], X.shape[1], Y.shape[1]
    Xs = torch.sum(X**2, dim=2)
    Ys = torch.sum(Y**2, dim=2)
    dist = -2.0 * torch.einsum("ipk,jqk->ijpq", X, Y)
    dist += torch.reshape(Xs, (A, 1, M, 1)) + torch.reshape(Ys, (1, B, 1, N))
    return dist


# Device launches of fewer distance elements than this keep the torch median (0: every device launch with `bw_median` takes
# `ops.path_sqdist_select`; DESIGN.md section 5.14 has the measurement behind the value)
MEDIAN_DEVICE_MIN_ELEMS = 0


def _median_keywords(get_bandwidth):
    """-> the `bw_scale` / `tol` keywords if `get_bandwidth` is `utils.math.bw_median` itself or a `functools.partial` of it
    with those keywords alone, else None"""
    import functools

    from .utils.math import bw_median

    if get_bandwidth is bw_median:
        return {}
    if (isinstance(get_bandwidth, functools.partial) and get_bandwidth.func is bw_median and not get_bandwidth.args
            and set(get_bandwidth.keywords) <= {"bw_scale", "tol"}):
        return dict(get_bandwidth.keywords)
    return None


def _median_route(get_bandwidth, on_device: bool, nelem: int) -> bool:
    """True where a data-dependent bandwidth is computed without the distance tensor: the function is the median heuristic
    (`_median_keywords`), the paths are on the device and the launch has at least MEDIAN_DEVICE_MIN_ELEMS distance elements.
    The median then comes from `ops.path_sqdist_select` (csrc/sqdist_select.hip) at any size.  Everything else -- CPU
    tensors, any other data-dependent function -- gets the [A,B,TX,TY] tensor from torch, up to _MAX_DIST_BYTES."""
    return bool(on_device) and nelem >= MEDIAN_DEVICE_MIN_ELEMS and _median_keywords(get_bandwidth) is not None


def _dist_elems(X, Y) -> int:
    return X.shape[0] * Y.shape[0] * X.shape[1] * Y.shape[1]


def _on_device(X, Y) -> bool:
    return X.device.type == "cuda" and Y.device.type == "cuda"


def _same_storage(X, Y) -> bool:
    """one tensor in both slots: the same elements at the same addresses"""
    return Y.data_ptr() == X.data_ptr() and Y.shape == X.shape and Y.stride() == X.stride() and Y.dtype == X.dtype


def inv_bandwidth_from_fn(get_bandwidth, X, Y) -> float:
    """1/h for the fused HIP path from a reference-style bandwidth function.  Constant functions are
    resolved without forming the distance tensor; the median heuristic on device tensors takes the median from
    `ops.path_sqdist_select` (`_median_route`); other data-dependent ones get the
    real [A,B,T,T] fp64 tensor, exactly what the reference passes (_traj_kernels.py:191-194)."""
    try:
        return 1.0 / float(get_bandwidth(_ConstantProbe()))
    except _ConstantProbe.Touched:
        pass
    nelem = _dist_elems(X, Y)
    if _median_route(get_bandwidth, _on_device(X, Y), nelem):
        from .utils.math import bw_from_median

        median = ops.path_sqdist_select(X.detach(), None if _same_storage(X, Y) else Y.detach())
        return 1.0 / float(bw_from_median(median, X.shape[0], **_median_keywords(get_bandwidth)))
    nbytes = nelem * 8
    if nbytes > _MAX_DIST_BYTES:
        raise RuntimeError(
            f"data-dependent bandwidth needs the full distance tensor ({nbytes / 2**30:.1f} GiB here); "
            "pass a constant bandwidth_fn (e.g. lambda _: h) for batches this large"
        )
    return 1.0 / float(get_bandwidth(gram_sqdist(X.detach().double(), Y.detach().double())))


def _resolve_static(static_kernel, X, Y):
    """-> (static_kind, inv_h) for the fused kernels, or (None, None) for a user static kernel.  Fused: this module's
    kernels, anything exposing `static_kind` + `inv_bandwidth` (sigsvgd_amd.kernels.BatchGaussianKernel) and the
    REFERENCE's own unpatched `BatchGaussianKernel` (recognised by `get_bandwidth` + `Gram_matrix`; it is an RBF with
    exp(-dist/h), src/kernels/_traj_kernels.py:176-195).  User: any other object with `Gram_matrix` (its grid goes
    through ops.PDESolve).  Anything else raises NotImplementedError before any device work."""
    if hasattr(static_kernel, "static_kind") and hasattr(static_kernel, "inv_bandwidth"):
        return int(static_kernel.static_kind), float(static_kernel.inv_bandwidth(X, Y))
    if type(static_kernel).__name__ == "BatchGaussianKernel" and hasattr(static_kernel, "get_bandwidth"):
        return _lib.STATIC_RBF, inv_bandwidth_from_fn(static_kernel.get_bandwidth, X, Y)
    if hasattr(static_kernel, "Gram_matrix"):
        return None, None
    raise NotImplementedError(
        f"static kernel {type(static_kernel).__name__} is not supported by the HIP path: it needs upstream's "
        "Gram_matrix(X, Y) (fused: RBFKernel, LinearKernel, IMQStaticKernel, RationalQuadraticKernel, Matern32StaticKernel, "
        "Matern52StaticKernel, BatchGaussianKernel, BatchIMQKernel, BatchRationalQuadraticKernel, BatchMatern32Kernel, "
        "BatchMatern52Kernel)"
    )


def _fp32_kw(fp32_sweeps) -> dict:
    """the `fp32_sweeps` keyword of the fused launches and queries, handed over only where it is set (a default SigKernel
    calls `ops` exactly as it did before the keyword existed)"""
    return {"fp32_sweeps": True} if fp32_sweeps else {}


def _exact_kw(exact_grad) -> dict:
    """the `exact_adjoint` keyword of the long route's gradient launches and queries (and `ops.PDESolve`'s trailing argument),
    handed over only where it is set, as `_fp32_kw`"""
    return {"exact_adjoint": True} if exact_grad else {}


def _nan_kw(nan_tails) -> dict:
    """the `nan_tails` keyword of the long route's launches and queries, handed over only where it is
    set, as `_exact_kw`"""
    return {"nan_tails": True} if nan_tails else {}


def _log_kw(log_k) -> dict:
    """the `log_k` keyword of the long route's launches and queries, handed over only where it is set,
    as `_exact_kw`"""
    return {"log_k": True} if log_k else {}


# ------------------------------------------------------------------------------------------------
# batches of paths of different lengths
# ------------------------------------------------------------------------------------------------
def _lengths_tensor(lengths, P, name):
    """lengths of the paths of P [A, T, d] -> int64 [A] on P's device, or None for None.  A sequence or a CPU tensor is checked
    here (integers, 1 <= L <= T: ValueError); a device tensor is checked for its shape and dtype alone and clamped to [1, T] on
    the device, because reading its values would be a host sync."""
    if lengths is None:
        return None
    A, T = P.shape[0], P.shape[1]
    if isinstance(lengths, torch.Tensor):
        if lengths.dim() != 1 or lengths.shape[0] != A:
            raise ValueError(f"{name} must be [{A}] (one length per path), got {tuple(lengths.shape)}")
        if lengths.dtype.is_floating_point or lengths.dtype.is_complex or lengths.dtype == torch.bool:
            raise ValueError(f"{name} must hold integers, got {lengths.dtype}")
        if lengths.device.type != "cpu":
            return lengths.detach().to(device=P.device, dtype=torch.int64).clamp(1, T)
        values = lengths.tolist()
    else:
        values = list(lengths)
        if len(values) != A:
            raise ValueError(f"{name} must hold {A} lengths (one per path), got {len(values)}")
        if any(isinstance(v, bool) or int(v) != v for v in values):
            raise ValueError(f"{name} must hold integers, got {values}")
    if any(not 1 <= int(v) <= T for v in values):
        raise ValueError(f"{name}: every length must be in [1, {T}] (the paths have {T} points), got {values}")
    return torch.tensor([int(v) for v in values], dtype=torch.int64).to(P.device, non_blocking=True)


def _same_lengths(lengths_X, lengths_Y) -> bool:
    """whether two `lengths` arguments are known to be equal without reading a device tensor: one object (None included), or
    equal host values"""
    if lengths_X is lengths_Y:
        return True
    if lengths_X is None or lengths_Y is None:
        return False
    on_host = lambda v: not isinstance(v, torch.Tensor) or v.device.type == "cpu"
    if on_host(lengths_X) and on_host(lengths_Y):
        return [int(v) for v in lengths_X] == [int(v) for v in lengths_Y]
    return isinstance(lengths_X, torch.Tensor) and isinstance(lengths_Y, torch.Tensor) and _same_storage(lengths_X, lengths_Y)


def _nan_tailed(P, L):
    """P with the points from each path's length on replaced by NaN: what SIGSVGD_FLAG_NAN_TAILS reads.  Built on P's device
    without a sync; autograd sends a gradient back to the kept entries only."""
    if L is None:
        return P
    keep = torch.arange(P.shape[1], device=P.device)[None, :] < L[:, None]
    return torch.where(keep[:, :, None], P, torch.full((), float("nan"), dtype=P.dtype, device=P.device))


def _lengths_static(kernel, X, Y):
    """-> (static_kind, inv_h) of a call with lengths, and its refusals: an explicit bandwidth only (padding would distort one
    computed from the data), built-in static kernels only, no learned sigma, no exact gradient, no fp32 sweeps"""
    sk = kernel.static_kernel
    if kernel.fp32_sweeps:
        raise ValueError("lengths run on the long route's fp64 sweeps; fp32_sweeps=True selects a fused fp32-sweep kernel")
    if kernel.exact_grad:
        raise NotImplementedError("lengths with exact_grad=True: the exact adjoint's kernels solve every pair on the launch's "
                                  "grid (SIGSVGD_FLAG_NAN_TAILS with SIGSVGD_FLAG_EXACT_ADJOINT is not built)")
    if _learned_sigma(sk) is not None:
        raise NotImplementedError("lengths with a static-kernel sigma that requires grad: the bandwidth launches do not take "
                                  "SIGSVGD_FLAG_NAN_TAILS")
    builtin = hasattr(sk, "static_kind") and hasattr(sk, "inv_bandwidth")
    reference_rbf = type(sk).__name__ == "BatchGaussianKernel" and hasattr(sk, "get_bandwidth")
    if not (builtin or reference_rbf):
        if hasattr(sk, "Gram_matrix"):
            raise NotImplementedError(f"lengths with the user static kernel {type(sk).__name__}: its grid is the caller's torch "
                                      "code; the built-in static kernels take lengths")
        return _resolve_static(sk, X, Y)  # (raises NotImplementedError)
    if hasattr(sk, "get_bandwidth"):
        try:
            return (int(sk.static_kind) if builtin else _lib.STATIC_RBF), 1.0 / float(sk.get_bandwidth(_ConstantProbe()))
        except _ConstantProbe.Touched:
            raise ValueError("lengths need an explicit bandwidth: one computed from the data (the median heuristic, any "
                             "bandwidth_fn that reads the distances) would see the padding.  Pass a constant bandwidth_fn "
                             "(lambda _: h) or a static kernel with a sigma") from None
    return int(sk.static_kind), float(sk.inv_bandwidth(X, Y))


def _long_route(X, Y, static_kind, dyadic_order, want_grad, naive, sym, y_is_x, fp32_sweeps=False) -> bool:
    """True where the fused Gram kernels refuse the launch (`ops.gram_takes`: their per-pair state outgrows the LDS); the
    built-in static kernels then run on the long route (`ops.gram_long_fwd*`, csrc/gram_long.hip).  Every launch the
    fused kernels take stays on them."""
    T = max(X.shape[1], Y.shape[1])  # (the fused route pads the shorter batch to this length)
    return not ops.gram_takes(X.shape[0], Y.shape[0], T, X.shape[2], dyadic_order, static_kind, want_grad, naive, sym, y_is_x,
                              **_fp32_kw(fp32_sweeps))


def _long_yx_route(y_is_x: bool, A: int, want_grad: bool, cus: int) -> bool:
    """True where a long-route launch with Y = X solves each unordered pair once (`ops.gram_long_fwd_bwd2`, y_is_x) instead
    of every ordered pair (`ops.gram_long_fwd*`).  Measured on the MI355X: the gradient launch wins
    where its work items are single pairs (A = 16, 32, 33: 1.36 to 1.51 times faster) and loses to the ordered launch where
    they are tiles whose count just passes the resident waves (A = 64, T = 300: 528 tiles of 2 x 2 for 512 waves, 0.91);
    the forward-only launch ties while a wave has one pair either way (A = 16, 32) and wins from A = 64 on.  So: gradient
    launches where the tiles of 2 x 2 would not give every compute unit one (single pairs then, whatever the LDS lets a
    unit hold: A <= 44 at 256 units); forward-only launches where the unordered pairs alone fill 8 waves per unit."""
    if not y_is_x:
        return False
    if want_grad:
        half = (A + 1) // 2
        return half * (half + 1) // 2 < cus
    return A * (A + 1) // 2 >= 8 * cus


def _device_cus(X) -> int:
    return torch.cuda.get_device_properties(X.device).multi_processor_count if X.is_cuda else 256


def _pair_route(A, TX, TY, d, static_kind, dyadic_order, want_grad, naive, cus, fp32_sweeps=False) -> bool:
    """True where `compute_kernel` with a built-in static kernel solves its pairs on the paired route (`ops.pair_fwd*`): every
    shape `ops.pair_takes` takes, except forward-only calls of A^2 <= cus pairs that the fused Gram kernels take.  Such a Gram
    launch is one round of the device, latency-bound like the paired launch but on the fused kernels' fp32 sweeps, so its
    diagonal is the faster forward there (A = 6, T = 100, order 3: 1.23 ms against 1.31 ms)."""
    if not ops.pair_takes(A, TX, TY, d, dyadic_order, static_kind, want_grad):
        return False
    if want_grad or A * A > cus:
        return True
    return not ops.gram_takes(A, A, max(TX, TY), d, dyadic_order, static_kind, False, naive, **_fp32_kw(fp32_sweeps))


def _solve_gram(X, Y, cfg, grad_out, want_x, want_y, fused_yx):
    """-> (K, gX or None, gY or None): the one place that chooses the launch of a Gram request with a built-in static kernel.
    cfg = (static_kind, inv_h, dyadic_order, naive, sym, y_is_x, fp32_sweeps); want_x / want_y: the gradients wanted (neither: forward
    only, grad_out unused); fused_yx: whether a gradient launch of the fused kernels with Y = X is told so (the speculated
    unit-weight launch and `gram_and_grad` are, a backward with real weights is not).

    The fused kernels take every launch `ops.gram_takes` grants; the long route takes the rest, each unordered pair once
    where `_long_yx_route` says so.  The long route gets K and both gradients from one `ops.gram_long_fwd_bwd2` launch (one
    solve per pair).  The fused route has no second-slot kernel: gY is the first slot of the swapped launch
    `ops.gram_fwd_bwd(Y, X, grad_out^T)`, a second launch.  fp32_sweeps (`SigKernel(..., fp32_sweeps=True)`) goes to the
    fused launches and their queries; the long route has no such kernels and does not see it.  An eighth element of cfg,
    exact_grad (`SigKernel(..., exact_grad=True)`): every gradient launch is the long route's with
    `exact_adjoint=True`, whatever the shape (the fused kernels have the GG convention only); forward-only launches are
    untouched.  A ninth, nan_tails (a call with lengths): X and Y are NaN-padded and every request,
    forward or gradient, is one `ops.gram_long_fwd_bwd2` launch with `nan_tails=True`, whatever the shape."""
    static_kind, inv_h, dyadic_order, naive, sym, y_is_x, fp32_sweeps, *rest = cfg
    exact = bool(rest and rest[0])
    fkw = _fp32_kw(fp32_sweeps)
    if len(rest) > 1 and rest[1]:  # nan_tails (a call with lengths): the flagged two-sided launch alone
        yx = y_is_x and not want_y
        if not ops.gram_long2_takes(X.shape[0], Y.shape[0], X.shape[1], Y.shape[1], X.shape[2], dyadic_order, static_kind,
                                    want_x, want_y, yx, nan_tails=True):
            raise _refused("compute_Gram", X, Y, dyadic_order, "a batch with lengths")
        return ops.gram_long_fwd_bwd2(X, Y, inv_h, dyadic_order, static_kind, grad_out, naive, sym, yx, want_x, want_y,
                                      nan_tails=True)
    if not (want_x or want_y):
        if not _long_route(X, Y, static_kind, dyadic_order, False, naive, False, y_is_x, fp32_sweeps):
            return ops.gram_fwd(X, Y, inv_h, dyadic_order, static_kind, naive, y_is_x=y_is_x, **fkw), None, None
        if _long_yx_route(y_is_x, X.shape[0], False, _device_cus(X)):
            return ops.gram_long_fwd_bwd2(X, Y, inv_h, dyadic_order, static_kind, None, naive, y_is_x=True,
                                          want_gradX=False, want_gradY=False)
        return ops.gram_long_fwd(X, Y, inv_h, dyadic_order, static_kind, naive), None, None
    yx = y_is_x and not want_y  # (one tensor in both slots with grad_Y: both slots of every ordered pair)
    if exact:
        if not ops.gram_long2_takes(X.shape[0], Y.shape[0], X.shape[1], Y.shape[1], X.shape[2], dyadic_order, static_kind,
                                    want_x, want_y, yx, exact_adjoint=True):
            raise _refused("compute_Gram", X, Y, dyadic_order, "the exact gradient (exact_grad=True)")
        if want_y or _long_yx_route(yx, X.shape[0], True, _device_cus(X)):
            return ops.gram_long_fwd_bwd2(X, Y, inv_h, dyadic_order, static_kind, grad_out, naive, sym, yx, want_x, want_y,
                                          exact_adjoint=True)
        return (*ops.gram_long_fwd_bwd(X, Y, inv_h, dyadic_order, static_kind, grad_out, naive, sym, exact_adjoint=True), None)
    if _long_route(X, Y, static_kind, dyadic_order, True, naive, sym, yx and fused_yx, fp32_sweeps):
        if want_y or _long_yx_route(yx, X.shape[0], True, _device_cus(X)):
            return ops.gram_long_fwd_bwd2(X, Y, inv_h, dyadic_order, static_kind, grad_out, naive, sym, yx, want_x, want_y)
        return (*ops.gram_long_fwd_bwd(X, Y, inv_h, dyadic_order, static_kind, grad_out, naive, sym), None)
    K = gX = gY = None
    if want_x:
        K, gX = ops.gram_fwd_bwd(X, Y, inv_h, dyadic_order, static_kind, grad_out, naive, sym, yx and fused_yx, **fkw)
    if want_y:  # the second slot is the first slot of the swapped launch
        Kt, gY = ops.gram_fwd_bwd(Y, X, inv_h, dyadic_order, static_kind, None if grad_out is None else grad_out.T, naive,
                                  False, False, **fkw)
        K = Kt.T.contiguous() if K is None else K
    return K, gX, gY


def _scaled_ones(g_ones, gy_ones, grad_output):
    """-> (gX, gY) from the unit-weight gradients speculated in forward where grad_output is uniform (an expanded scalar, or
    equal entries: one host sync), each None where it was not speculated; (None, None) for any other grad_output"""
    if g_ones is None and gy_ones is None:
        return None, None
    scalar = grad_output.reshape(-1)[:1]
    # an expanded scalar (e.g. from K.sum().backward()) is uniform as it stands; anything else costs one host sync
    if grad_output.stride() != (0, 0) and not bool((grad_output == scalar).all()):
        return None, None
    return (None if g_ones is None else g_ones * scalar.to(g_ones.dtype),
            None if gy_ones is None else gy_ones * scalar.to(gy_ones.dtype))


# ------------------------------------------------------------------------------------------------
# autograd node
# ------------------------------------------------------------------------------------------------
class _SigKernelGram(torch.autograd.Function):
    """forward: K = Gram(X, Y).  backward: d sum(grad_output*K)/dX, and with grad_Y d sum(grad_output*K)/dY (the second
    slot), else nothing for Y.

    When X (or, with grad_Y, Y) needs a gradient the forward already runs the forward+backward kernel for
    grad_output = 1 (the only grad_output the reference ever produces: callers differentiate
    K.sum(), score.py:69 / trajectory_svgd.py:65), so the usual backward is a scale by a scalar.
    Any other grad_output triggers one more launch with the real weights.  `_solve_gram` chooses every launch."""

    @staticmethod
    def forward(ctx, X, Y, static_kind, inv_h, dyadic_order, naive, sym, y_is_x, speculate, grad_Y, fp32_sweeps=False,
                exact_grad=False, nan_tails=False):
        ctx.cfg = (static_kind, inv_h, dyadic_order, naive, sym, y_is_x, fp32_sweeps, exact_grad, nan_tails)
        ctx.g_ones = ctx.gy_ones = None
        ctx.want = (ctx.needs_input_grad[0], bool(grad_Y) and ctx.needs_input_grad[1])
        ctx.y_dtype = Y.dtype
        Xd = X.detach()
        Yd = Y.detach()
        if any(ctx.want) and speculate:
            K, ctx.g_ones, ctx.gy_ones = _solve_gram(Xd, Yd, ctx.cfg, None, *ctx.want, True)
        else:
            K = _solve_gram(Xd, Yd, ctx.cfg, None, False, False, False)[0]
        ctx.save_for_backward(Xd, Yd)
        return K

    @staticmethod
    def backward(ctx, grad_output):
        X, Y = ctx.saved_tensors
        want_x, want_y = ctx.want
        gX, gY = _scaled_ones(ctx.g_ones, ctx.gy_ones, grad_output)
        if gX is None and gY is None and (want_x or want_y):
            _, gX, gY = _solve_gram(X, Y, ctx.cfg, grad_output, want_x, want_y, False)
        if gY is not None:
            gY = gY.to(ctx.y_dtype)
        return gX, gY, None, None, None, None, None, None, None, None, None, None, None


class _SigKernelPair(torch.autograd.Function):
    """forward: K[i] = k_sig(X_i, Y_i) (`ops.pair_fwd*`, one solve per pair).  backward: X and Y each get the derivative of
    their own slot (a tensor passed in both slots gets the sum from autograd).

    When X or Y needs a gradient the forward runs `ops.pair_fwd_bwd` with unit weights for the outputs needed: pair i's
    gradient is linear in its own weight alone, so backward scales row i by grad_output[i] (exact up to one rounding) and
    there is one launch per call.  The launch computes in X's dtype; each gradient returns in its own input's dtype."""

    @staticmethod
    def forward(ctx, X, Y, static_kind, inv_h, dyadic_order, naive, exact_grad=False, nan_tails=False, log_k=False):
        want_x, want_y = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        ctx.dtypes = (X.dtype, Y.dtype)
        if want_x or want_y:
            K, gX, gY = ops.pair_fwd_bwd(X.detach(), Y.detach(), inv_h, dyadic_order, static_kind, None, naive, want_x,
                                         want_y, **_exact_kw(exact_grad), **_nan_kw(nan_tails), **_log_kw(log_k))
            ctx.save_for_backward(gX, gY)
        else:
            K = ops.pair_fwd(X.detach(), Y.detach(), inv_h, dyadic_order, static_kind, naive, **_nan_kw(nan_tails),
                             **_log_kw(log_k))
        return K

    @staticmethod
    def backward(ctx, grad_output):
        gX1, gY1 = ctx.saved_tensors
        gX = gY = None
        if gX1 is not None:
            gX = (gX1 * grad_output.to(gX1.dtype)[:, None, None]).to(ctx.dtypes[0])
        if gY1 is not None:
            gY = (gY1 * grad_output.to(gY1.dtype)[:, None, None]).to(ctx.dtypes[1])
        return gX, gY, None, None, None, None, None, None, None


# ------------------------------------------------------------------------------------------------
# log-domain and normalised kernels
# ------------------------------------------------------------------------------------------------
def _log_forward(X, Y, cfg, y_is_x):
    """ln K [A, B]: the flagged two-sided launch, forward only"""
    static_kind, inv_h, dyadic_order = cfg
    return ops.gram_long_fwd_bwd2(X, Y, inv_h, dyadic_order, static_kind, None, False, False, y_is_x, False, False,
                                  log_k=True)[0]


class _SigKernelLogGram(torch.autograd.Function):
    """forward: ln K = log Gram(X, Y), one flagged two-sided launch (`ops.gram_long_fwd_bwd2(..., log_k=True)`), forward only.
    backward: one flagged launch with grad_out = grad_output, which returns d sum(grad_output ln K) / dX and, with grad_Y, / dY."""

    @staticmethod
    def forward(ctx, X, Y, static_kind, inv_h, dyadic_order, sym, y_is_x, grad_Y):
        ctx.cfg = (static_kind, inv_h, dyadic_order)
        ctx.sym, ctx.y_is_x, ctx.y_dtype = sym, y_is_x, Y.dtype
        ctx.want = (ctx.needs_input_grad[0], bool(grad_Y) and ctx.needs_input_grad[1])
        Xd, Yd = X.detach(), Y.detach()
        ctx.save_for_backward(Xd, Yd)
        return _log_forward(Xd, Yd, ctx.cfg, y_is_x)

    @staticmethod
    def backward(ctx, grad_output):
        X, Y = ctx.saved_tensors
        static_kind, inv_h, dyadic_order = ctx.cfg
        want_x, want_y = ctx.want
        gX = gY = None
        if want_x or want_y:
            _, gX, gY = ops.gram_long_fwd_bwd2(X, Y, inv_h, dyadic_order, static_kind, grad_output, False, ctx.sym,
                                               ctx.y_is_x and not want_y, want_x, want_y, log_k=True)
        if gY is not None:
            gY = gY.to(ctx.y_dtype)
        return gX, gY, None, None, None, None, None, None


class _SigKernelNormGram(torch.autograd.Function):
    """The normalised Gram matrix Khat_ij = K(X_i, Y_j) / sqrt(K(X_i, X_i) K(Y_j, Y_j)) = exp(l_ij - a_i / 2 - b_j / 2) from the
    logarithms alone, so that it exists where K itself overflows.

    forward: l from one flagged two-sided launch, a and b from flagged paired launches on (X, X) and (Y, Y) (one where one
    tensor is in both slots); all forward only.  The paired and the two-sided launch give ln K the same bits, so the diagonal of
    Khat(X, X) is exactly 1.
    backward, for upstream G with W = G * Khat: one flagged two-sided launch with grad_out = W, and per batch that is
    differentiated one flagged `ops.pair_fwd_bwd` with grad_out = -rowsum(W) / 2 (X) or -colsum(W) / 2 (Y), whose gX + gY is
    added.  sym (one batch in both slots, gradient folded into the first): the two-sided launch weights W + W^T and the paired
    launch on X carries both sums.  No host sync anywhere."""

    @staticmethod
    def forward(ctx, X, Y, static_kind, inv_h, dyadic_order, sym, y_is_x, grad_Y):
        ctx.cfg = (static_kind, inv_h, dyadic_order)
        ctx.sym, ctx.y_is_x, ctx.y_dtype = sym, y_is_x, Y.dtype
        ctx.want = (ctx.needs_input_grad[0], bool(grad_Y) and ctx.needs_input_grad[1])
        Xd, Yd = X.detach(), Y.detach()
        l = _log_forward(Xd, Yd, ctx.cfg, y_is_x)
        a = ops.pair_fwd(Xd, Xd, inv_h, dyadic_order, static_kind, log_k=True)
        b = a if y_is_x else ops.pair_fwd(Yd, Yd, inv_h, dyadic_order, static_kind, log_k=True).to(a.dtype)
        Khat = torch.exp(l - (0.5 * a[:, None] + 0.5 * b[None, :]))  # (symmetric where l is; a - (a / 2 + a / 2) = 0 exactly)
        ctx.save_for_backward(Xd, Yd, Khat)
        return Khat

    @staticmethod
    def backward(ctx, grad_output):
        X, Y, Khat = ctx.saved_tensors
        static_kind, inv_h, dyadic_order = ctx.cfg
        want_x, want_y = ctx.want
        if not (want_x or want_y):
            return (None,) * 8
        W = grad_output * Khat
        _, gX, gY = ops.gram_long_fwd_bwd2(X, Y, inv_h, dyadic_order, static_kind, W, False, ctx.sym,
                                           ctx.y_is_x and not want_y, want_x, want_y, log_k=True)

        def diagonal_term(P, weights):  # d sum(weights ln K(P_i, P_i)) / dP: both slots
            _, pX, pY = ops.pair_fwd_bwd(P, P, inv_h, dyadic_order, static_kind, weights, log_k=True)
            return pX + pY

        if want_x:
            gX = gX + diagonal_term(X, -0.5 * (W.sum(1) + W.sum(0) if ctx.sym else W.sum(1)))
        if want_y:
            gY = (gY + diagonal_term(Y, -0.5 * W.sum(0))).to(ctx.y_dtype)
        return gX, gY, None, None, None, None, None, None


class _SigKernelNormFusedGram(torch.autograd.Function):
    """The normalised Gram matrix on the fused route (`SigKernel(normalize=True, normalize_route="fused")`, DESIGN.md section
    5.23).  forward: one `ops.gram_fwd(..., normalized=True)`.  backward: one `ops.gram_fwd_bwd(..., normalized=True)` with
    grad_out = grad_output, which returns d sum(grad_output * Khat) / dX, the diagonals' dependence included (first slot; sym:
    weights grad_output + grad_output^T).  Y gets no gradient."""

    @staticmethod
    def forward(ctx, X, Y, static_kind, inv_h, dyadic_order, sym, y_is_x, fp32_sweeps):
        ctx.cfg = (static_kind, inv_h, dyadic_order, sym, y_is_x, fp32_sweeps)
        Xd, Yd = X.detach(), Y.detach()
        ctx.save_for_backward(Xd, Yd)
        return ops.gram_fwd(Xd, Yd, inv_h, dyadic_order, static_kind, y_is_x=y_is_x, normalized=True, **_fp32_kw(fp32_sweeps))

    @staticmethod
    def backward(ctx, grad_output):
        X, Y = ctx.saved_tensors
        static_kind, inv_h, dyadic_order, sym, y_is_x, fp32_sweeps = ctx.cfg
        gX = None
        if ctx.needs_input_grad[0]:
            gX = ops.gram_fwd_bwd(X, Y, inv_h, dyadic_order, static_kind, grad_output, sym=sym, y_is_x=y_is_x, normalized=True,
                                  **_fp32_kw(fp32_sweeps))[1]
        return gX, None, None, None, None, None, None, None


# ------------------------------------------------------------------------------------------------
# a static-kernel sigma that requires grad
# ------------------------------------------------------------------------------------------------
def _learned_sigma(static_kernel):
    """-> the static kernel's `sigma` where it is to be differentiated: one of this module's RBF / IMQ / rational-quadratic /
    Matern kernels whose sigma is a one-element tensor that requires grad, with grad mode on.  None otherwise (a float, a plain
    tensor, `torch.no_grad()`, any other static kernel): those calls take the launches they always took."""
    if not isinstance(static_kernel, (RBFKernel, IMQStaticKernel, Matern32StaticKernel)) or not torch.is_grad_enabled():
        return None
    sigma = getattr(static_kernel, "sigma", None)
    if not isinstance(sigma, torch.Tensor) or not sigma.requires_grad:
        return None
    if sigma.numel() != 1:
        raise ValueError(f"a static-kernel sigma that requires grad must have one element, got {tuple(sigma.shape)}")
    return sigma


def _sigma_grad(sigma_like, inv_h, grad_output, dK_dinvh):
    """d sum(grad_output K) / d sigma from the saved per-pair dK / d inv_h (inv_h = 1 / sigma): no launch"""
    g = -(inv_h * inv_h) * (grad_output.double() * dK_dinvh.double()).sum()
    return g.to(device=sigma_like.device, dtype=sigma_like.dtype).reshape(sigma_like.shape)


def _refused(what, X, Y, dyadic_order, whose="the gradient of a static-kernel sigma"):
    return NotImplementedError(
        f"{what}: {whose} runs on the long route only (csrc/gram_long.hip), which refuses "
        f"paths {tuple(X.shape)} x {tuple(Y.shape)} at dyadic order {dyadic_order}: {_lib.last_error()}")


class _SigKernelGramSigma(torch.autograd.Function):
    """`_SigKernelGram` with the static kernel's sigma as an input: every launch is the long route's bandwidth launch
    (`ops.gram_long_fwd_bwd_h`), whose per-pair dK / d inv_h is saved in forward; backward returns
    grad_sigma = -inv_h^2 sum(grad_output dK_dinvh) without a launch.  X and Y keep `_SigKernelGram`'s rules: the unit-weight
    gradients are speculated in forward, a non-uniform grad_output takes one `ops.gram_long_fwd_bwd2` launch with the real
    weights (the same bits as the bandwidth launch returns)."""

    @staticmethod
    def forward(ctx, X, Y, sigma, static_kind, inv_h, dyadic_order, naive, sym, y_is_x, speculate, grad_Y, exact_grad=False):
        ctx.exact_kw = _exact_kw(exact_grad)
        ctx.want = (ctx.needs_input_grad[0], bool(grad_Y) and ctx.needs_input_grad[1])
        ctx.yx = y_is_x and not ctx.want[1]  # (one tensor in both slots with grad_Y: both slots of every ordered pair)
        ctx.cfg = (static_kind, inv_h, dyadic_order, naive, sym)
        ctx.y_dtype = Y.dtype
        ctx.sigma_like = sigma.detach()
        Xd, Yd = X.detach(), Y.detach()
        spec = speculate and any(ctx.want)
        K, ctx.g_ones, ctx.gy_ones, dK = ops.gram_long_fwd_bwd_h(Xd, Yd, inv_h, dyadic_order, static_kind, None, naive, sym,
                                                                 ctx.yx, spec and ctx.want[0], spec and ctx.want[1],
                                                                 **ctx.exact_kw)
        ctx.save_for_backward(Xd, Yd, dK)
        return K

    @staticmethod
    def backward(ctx, grad_output):
        X, Y, dK = ctx.saved_tensors
        static_kind, inv_h, dyadic_order, naive, sym = ctx.cfg
        want_x, want_y = ctx.want
        gS = _sigma_grad(ctx.sigma_like, inv_h, grad_output, dK) if ctx.needs_input_grad[2] else None
        gX, gY = _scaled_ones(ctx.g_ones, ctx.gy_ones, grad_output)
        if gX is None and gY is None and (want_x or want_y):
            _, gX, gY = ops.gram_long_fwd_bwd2(X, Y, inv_h, dyadic_order, static_kind, grad_output, naive, sym, ctx.yx,
                                               want_x, want_y, **ctx.exact_kw)
        if gY is not None:
            gY = gY.to(ctx.y_dtype)
        return gX, gY, gS, None, None, None, None, None, None, None, None, None


class _SigKernelPairSigma(torch.autograd.Function):
    """`_SigKernelPair` with the static kernel's sigma as an input: one `ops.pair_fwd_bwd_h` launch in forward (unit weights,
    the coordinate gradients needed, the per-pair dK / d inv_h), and a backward without launches."""

    @staticmethod
    def forward(ctx, X, Y, sigma, static_kind, inv_h, dyadic_order, naive, exact_grad=False):
        want_x, want_y = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        ctx.dtypes = (X.dtype, Y.dtype)
        ctx.inv_h = inv_h
        ctx.sigma_like = sigma.detach()
        K, gX, gY, dK = ops.pair_fwd_bwd_h(X.detach(), Y.detach(), inv_h, dyadic_order, static_kind, None, naive, want_x,
                                           want_y, **_exact_kw(exact_grad))
        ctx.save_for_backward(gX, gY, dK)
        return K

    @staticmethod
    def backward(ctx, grad_output):
        gX1, gY1, dK = ctx.saved_tensors
        gX = gY = gS = None
        if gX1 is not None:
            gX = (gX1 * grad_output.to(gX1.dtype)[:, None, None]).to(ctx.dtypes[0])
        if gY1 is not None:
            gY = (gY1 * grad_output.to(gY1.dtype)[:, None, None]).to(ctx.dtypes[1])
        if ctx.needs_input_grad[2]:
            gS = _sigma_grad(ctx.sigma_like, ctx.inv_h, grad_output, dK)
        return gX, gY, gS, None, None, None, None, None


class SigKernel:
    """Signature kernel with a static kernel and a dyadic refinement order (PDE solver).

    fp32_sweeps=True: `IMQStaticKernel` and `RationalQuadraticKernel` Gram launches at dyadic order 0,
    3 <= T <= 64, d <= 16 run on the register-resident fp32-sweep kernel RBF runs there (K per entry within 1e-5, the gradient
    within 1e-5 of its largest entry) instead of the fp64 coverage kernel, and so do `RBFKernel` launches of 17 <= d <= 32
    channels at order 0, 3 <= T <= 64 (section 5.25; RBF at d <= 16 runs there by default); everything else is unchanged.  It reaches the fused
    Gram launches only: the long route, the paired route of `compute_kernel` and a learned sigma (a `sigma` tensor that requires
    grad takes the long route's bandwidth launch, section 5.16) ignore it.

    exact_grad=True: every gradient -- of X, of Y, of a learned sigma, of a user static kernel's grid --
    is the exact derivative of the discrete K the call returns (the adjoint of the default second-order stencil itself), where
    the default is the reference's GG convention, which differs from it by per cents and is the gradient of no function: what
    `compute_mmd(grad_Y=True)` training, a learned sigma, line-search optimisers and `torch.autograd.gradcheck` need.  Every
    gradient-bearing launch of `compute_Gram`, `compute_kernel`, `compute_distance`, `compute_mmd` and `gram_and_grad` then
    takes the long route with SIGSVGD_FLAG_EXACT_ADJOINT whatever the shape (fp64 sweeps; K keeps the long route's bits);
    shapes the long route refuses raise NotImplementedError.  Forward-only calls are untouched, and so is `_naive_solver=True`,
    whose GG is exact already.  Not together with fp32_sweeps (ValueError).

    normalize=True: `compute_Gram`, `compute_kernel`, `compute_distance` and `compute_mmd` return the
    normalised kernel K(x, y) / sqrt(K(x, x) K(y, y)), built from the log-domain launches of the long route
    (SIGSVGD_FLAG_LOG_K), so it exists and is differentiable where K itself overflows (K(x, x) of rough paths passes fp32 from
    about 300 points and fp64 from about 1600).  Whatever the shape, these calls run on the long route at its fp64 cost, as
    exact_grad=True does; shapes it refuses, `lengths_*`, exact_grad=True, `_naive_solver=True`, a sigma that requires grad and
    user static kernels raise NotImplementedError, fp32_sweeps=True ValueError.  `compute_log_Gram` and `compute_log_kernel`
    return ln K itself (with any value of normalize).  `gram_and_grad` with normalize=True returns the
    normalised Gram matrix and the gradient of sum(grad_out * K^) in X from exactly one launch of the long route
    (`ops.gram_long_fwd_bwd2(..., normalized=True)`, SIGSVGD_FLAG_NORMALIZED: each pair solved once), whatever the shape; with
    Y None that is the gradient at fixed second slot, which SVGD uses.  The same refusals.

    normalize=True, normalize_route="fused" (the default "long" is everything above, unchanged):
    `gram_and_grad` is exactly one `ops.gram_fwd_bwd(..., normalized=True)` (SIGSVGD_FLAG_NORMALIZED_FUSED: the normalisation
    around the unflagged fused launch, at that launch's cost and accuracy), `compute_Gram` a node of `ops.gram_fwd` /
    `ops.gram_fwd_bwd` with the flag, `compute_mmd` follows through it; fp32_sweeps=True means there what it means without
    normalize.  For shapes whose K(x, x) fits the dtype (T <= 128 does).  grad_Y=True, `lengths_*`, a sigma that requires grad,
    user static kernels and shapes `ops.gram_takes` refuses raise NotImplementedError (exact_grad=True and _naive_solver=True
    do at construction).  `compute_kernel`, `compute_distance` and the `compute_log_*` methods keep the long route.
    normalize_route="fused" without normalize=True raises ValueError."""

    def __init__(self, static_kernel, dyadic_order: int, _naive_solver: bool = False, fp32_sweeps: bool = False,
                 exact_grad: bool = False, normalize: bool = False, normalize_route: str = "long"):
        if normalize_route not in ("long", "fused"):
            raise ValueError(f"SigKernel: normalize_route must be 'long' or 'fused', got {normalize_route!r}")
        if normalize_route == "fused" and not normalize:
            raise ValueError("SigKernel: normalize_route='fused' selects the route of the normalised kernel; it needs "
                             "normalize=True")
        if normalize and fp32_sweeps and normalize_route != "fused":
            raise ValueError("SigKernel: normalize=True runs on the long route's fp64 log-domain sweeps; fp32_sweeps=True "
                             "selects an fp32-sweep kernel.  Use one of them")
        if normalize and exact_grad:
            raise NotImplementedError("SigKernel: normalize=True with exact_grad=True: SIGSVGD_FLAG_LOG_K together with "
                                      "SIGSVGD_FLAG_EXACT_ADJOINT is not built")
        if normalize and _naive_solver:
            raise NotImplementedError("SigKernel: normalize=True with _naive_solver=True: the log-domain kernels have the "
                                      "default stencil only")
        if exact_grad and fp32_sweeps:
            raise ValueError("SigKernel: exact_grad=True runs every gradient launch on the long route's fp64 sweeps; "
                             "fp32_sweeps=True selects an fp32-sweep kernel.  Use one of them")
        self.static_kernel = static_kernel
        self.dyadic_order = int(dyadic_order)
        self._naive_solver = bool(_naive_solver)
        self.fp32_sweeps = bool(fp32_sweeps)
        self.exact_grad = bool(exact_grad)
        self.normalize = bool(normalize)
        self.normalize_route = normalize_route
        self.speculate_ones = True
        self.value_check_min_batch = 32  # below this a launch is latency-bound and the compare would not pay

    def compute_Gram(self, X: torch.Tensor, Y: torch.Tensor, sym: bool = False, grad_Y: bool = False, lengths_X=None,
                     lengths_Y=None) -> torch.Tensor:
        """K[i,j] = k_sig(X_i, Y_j), X [A,Tx,d], Y [B,Ty,d] on a HIP device; same dtype/device as X.  Paths of different
        lengths (upstream sigkernel takes them) are padded with their last point, which is exact (ops.pad_to_length).
        Gradients flow to X (the first slot).  grad_Y=True: a Y that requires grad receives its second-slot gradient too (one
        tensor in both slots then gets the sum of both, which is what sym=True gives; the two together raise ValueError).
        The default leaves Y without a gradient, as callers that pass one leaf tensor in both slots rely on.

        lengths_X [A] / lengths_Y [B] (integers in [1, T], a tensor on either device or a sequence; None: every path is
        whole): path i of X is its first lengths_X[i] points, whatever the rest of its row holds, and every pair is solved on
        its own grid (`_lengths_gram`).  The padded entries of X and Y get a zero gradient."""
        if grad_Y and sym:
            raise ValueError("compute_Gram: grad_Y=True differentiates the second slot itself; sym=True folds it into the "
                             "first.  Use one of them")
        if self.normalize and self.normalize_route == "fused":
            static_kind, inv_h = self._fused_norm_static("compute_Gram", X, Y, sym, _same_storage(X, Y), grad_Y, lengths_X,
                                                         lengths_Y)
            return _SigKernelNormFusedGram.apply(X, Y, static_kind, inv_h, self.dyadic_order, bool(sym), _same_storage(X, Y),
                                                 self.fp32_sweeps)
        if self.normalize:
            return self._log_gram(_SigKernelNormGram, "compute_Gram", X, Y, sym, grad_Y, lengths_X, lengths_Y)
        if lengths_X is not None or lengths_Y is not None:
            return self._lengths_gram(X, Y, bool(sym), bool(grad_Y), lengths_X, lengths_Y)
        static_kind, inv_h = _resolve_static(self.static_kernel, X, Y)
        if static_kind is None:  # user static kernel: its grid, the PDE on the device, autograd through both
            G = self.static_kernel.Gram_matrix(X, Y if sym or grad_Y else Y.detach())
            return ops.PDESolve.apply(G, self.dyadic_order, self._naive_solver, *_exact_kw(self.exact_grad).values())
        y_is_x = _same_storage(X, Y)
        if (not y_is_x and Y.shape == X.shape and Y.dtype == X.dtype and X.shape[0] >= self.value_check_min_batch
                and bool(torch.equal(X.detach(), Y.detach()))):
            # The reference's callers pass two BUFFERS with the same values -- `compute_Gram(X.double(),
            # Y.double())` with Y = x.detach() (src/kernels/_traj_kernels.py:205, src/inference/trajectory_svgd.py:60-62).
            # One device compare + scalar read-back (tens of microseconds) buys the symmetric solve: each
            # unordered pair once instead of every ordered pair, i.e. half the launch at these batch sizes.
            y_is_x = True
        sigma = _learned_sigma(self.static_kernel)
        if sigma is not None:  # the long route's bandwidth launch, whatever the shape
            want_y = bool(grad_Y) and Y.requires_grad
            if not ops.gram_long_h_takes(X.shape[0], Y.shape[0], X.shape[1], Y.shape[1], X.shape[2], self.dyadic_order,
                                         static_kind, X.requires_grad, want_y, self._naive_solver, y_is_x and not want_y,
                                         **_exact_kw(self.exact_grad)):
                raise _refused("compute_Gram", X, Y, self.dyadic_order)
            return _SigKernelGramSigma.apply(X, Y, sigma, static_kind, inv_h, self.dyadic_order, self._naive_solver,
                                             bool(sym), y_is_x, self.speculate_ones, bool(grad_Y),
                                             *_exact_kw(self.exact_grad).values())
        return _SigKernelGram.apply(X, Y, static_kind, inv_h, self.dyadic_order, self._naive_solver, bool(sym),
                                    y_is_x, self.speculate_ones, bool(grad_Y), self.fp32_sweeps,
                                    *_exact_kw(self.exact_grad).values())

    # -- the rest of the upstream `sigkernel.SigKernel` surface [RECALLED from the public package; the
    #    reference tree never calls these].  compute_kernel / compute_distance differentiate both arguments (each its
    #    own slot); compute_mmd goes through compute_Gram, so its cross term's gradient flows to the FIRST argument only
    #    unless grad_Y=True, with `sym=True` giving the symmetrised weighting for Gram(X, X).
    # -- batches of paths of different lengths -------------------------------------------------------
    def _lengths_operands(self, X, Y, sym, lengths_X, lengths_Y):
        """-> (static_kind, inv_h, Xn, Yn, y_is_x): the static kernel of a call with lengths (`_lengths_static`) and the NaN-padded
        operands, built once where one tensor with one set of lengths is in both slots"""
        if X.dim() != 3 or Y.dim() != 3:
            raise ValueError(f"paths must be [batch, length, dim]; got {tuple(X.shape)} and {tuple(Y.shape)}")
        static_kind, inv_h = _lengths_static(self, X, Y)
        LX, LY = _lengths_tensor(lengths_X, X, "lengths_X"), _lengths_tensor(lengths_Y, Y, "lengths_Y")
        same = _same_lengths(lengths_X, lengths_Y)
        if sym and not same:
            raise ValueError("sym=True weights K and its transpose alike, which needs one batch in both slots: lengths_X and "
                             "lengths_Y must be the same")
        y_is_x = same and _same_storage(X, Y)
        Xn = _nan_tailed(X, LX)
        return static_kind, inv_h, Xn, (Xn if y_is_x else _nan_tailed(Y, LY)), y_is_x

    def _lengths_gram(self, X, Y, sym, grad_Y, lengths_X, lengths_Y):
        """compute_Gram with lengths: the NaN-padded operands through `_SigKernelGram` with nan_tails set, so that every launch,
        forward or gradient, is `ops.gram_long_fwd_bwd2(..., nan_tails=True)`"""
        static_kind, inv_h, Xn, Yn, y_is_x = self._lengths_operands(X, Y, sym, lengths_X, lengths_Y)
        return _SigKernelGram.apply(Xn, Yn, static_kind, inv_h, self.dyadic_order, self._naive_solver, sym, y_is_x,
                                    self.speculate_ones, grad_Y, False, False, True)

    def _lengths_kernel(self, X, Y, lengths_X, lengths_Y):
        """compute_kernel with lengths: the NaN-padded operands on the paired route with nan_tails set, whatever the shape"""
        static_kind, inv_h, Xn, Yn, _ = self._lengths_operands(X, Y, False, lengths_X, lengths_Y)
        want_grad = torch.is_grad_enabled() and (Xn.requires_grad or Yn.requires_grad)
        if not ops.pair_takes(X.shape[0], X.shape[1], Y.shape[1], X.shape[2], self.dyadic_order, static_kind, want_grad,
                              nan_tails=True):
            raise _refused("compute_kernel", X, Y, self.dyadic_order, "a batch with lengths")
        return _SigKernelPair.apply(Xn, Yn, static_kind, inv_h, self.dyadic_order, self._naive_solver, False, True)

    # -- log-domain and normalised kernels -----------------------------------------------------------
    def _log_static(self, what, X, Y, lengths_X=None, lengths_Y=None):
        """-> (static_kind, inv_h) of a call that runs the log-domain launches, and its refusals"""
        if lengths_X is not None or lengths_Y is not None:
            raise NotImplementedError(f"{what}: lengths_X / lengths_Y with the log-domain launches: SIGSVGD_FLAG_LOG_K together "
                                      "with SIGSVGD_FLAG_NAN_TAILS is not built")
        if self.exact_grad or self._naive_solver:
            raise NotImplementedError(f"{what}: the log-domain launches have the default stencil's GG gradient only "
                                      "(not with exact_grad=True or _naive_solver=True)")
        if _learned_sigma(self.static_kernel) is not None:
            raise NotImplementedError(f"{what}: a static-kernel sigma that requires grad: the bandwidth launches do not take "
                                      "SIGSVGD_FLAG_LOG_K")
        static_kind, inv_h = _resolve_static(self.static_kernel, X, Y)
        if static_kind is None:
            raise NotImplementedError(f"{what}: the user static kernel {type(self.static_kernel).__name__} runs on "
                                      "ops.PDESolve, which has no log-domain form; the built-in static kernels have one")
        return static_kind, inv_h

    def _log_gram(self, node, what, X, Y, sym, grad_Y, lengths_X=None, lengths_Y=None):
        """the two-sided log-domain node (`_SigKernelLogGram` or `_SigKernelNormGram`) of a call, whatever the shape"""
        static_kind, inv_h = self._log_static(what, X, Y, lengths_X, lengths_Y)
        y_is_x = _same_storage(X, Y)
        if not ops.gram_long2_takes(X.shape[0], Y.shape[0], X.shape[1], Y.shape[1], X.shape[2], self.dyadic_order, static_kind,
                                    True, True, False, log_k=True):
            raise _refused(what, X, Y, self.dyadic_order, "the log-domain solve")
        return node.apply(X, Y, static_kind, inv_h, self.dyadic_order, bool(sym), y_is_x, bool(grad_Y))

    def compute_log_Gram(self, X: torch.Tensor, Y: torch.Tensor, sym: bool = False, grad_Y: bool = False) -> torch.Tensor:
        """ln K[i,j] = ln k_sig(X_i, Y_j) from the log-domain launch of the long route (SIGSVGD_FLAG_LOG_K), differentiable as
        `compute_Gram` is (sym, grad_Y as there): finite where K itself overflows.  NaN where the discrete K is <= 0."""
        if grad_Y and sym:
            raise ValueError("compute_log_Gram: grad_Y=True differentiates the second slot itself; sym=True folds it into the "
                             "first.  Use one of them")
        return self._log_gram(_SigKernelLogGram, "compute_log_Gram", X, Y, sym, grad_Y)

    def compute_log_kernel(self, X: torch.Tensor, Y: torch.Tensor) -> torch.Tensor:
        """ln k_sig(X_i, Y_i) -> [batch] from the paired log-domain launch, differentiable in X and in Y (each its own slot)."""
        assert X.shape[0] == Y.shape[0], "compute_log_kernel pairs X_i with Y_i"
        static_kind, inv_h = self._log_static("compute_log_kernel", X, Y)
        want_grad = torch.is_grad_enabled() and (X.requires_grad or Y.requires_grad)
        if not ops.pair_takes(X.shape[0], X.shape[1], Y.shape[1], X.shape[2], self.dyadic_order, static_kind, want_grad,
                              log_k=True):
            raise _refused("compute_log_kernel", X, Y, self.dyadic_order, "the log-domain solve")
        return _SigKernelPair.apply(X, Y, static_kind, inv_h, self.dyadic_order, False, False, False, True)

    def _normalized_kernel(self, X, Y, lengths_X, lengths_Y):
        """compute_kernel with normalize=True: exp(ln k(X_i, Y_i) - ln k(X_i, X_i) / 2 - ln k(Y_i, Y_i) / 2) of three paired
        log-domain launches (two where one tensor is in both slots of the call: then the result is exactly 1)"""
        self._log_static("compute_kernel", X, Y, lengths_X, lengths_Y)
        a = self.compute_log_kernel(X, X)
        if _same_storage(X, Y):
            return torch.exp(a - 0.5 * a - 0.5 * a)
        return torch.exp(self.compute_log_kernel(X, Y) - 0.5 * a - 0.5 * self.compute_log_kernel(Y, Y).to(a.dtype))

    def compute_kernel(self, X: torch.Tensor, Y: torch.Tensor, lengths_X=None, lengths_Y=None) -> torch.Tensor:
        """Paired kernel k_sig(X_i, Y_i) -> [batch], one solve per pair, differentiable in X and in Y (each its own slot:
        compute_kernel(X, X) differentiates to the sum of both).  Built-in static kernels run on the paired route
        (`ops.pair_fwd*`, csrc/gram_long.hip) wherever `_pair_route` says so, else on the diagonal of compute_Gram (first
        slot only) as before: where `ops.pair_takes` refuses the shape, and for forward-only calls of few pairs; a user static kernel with `batch_kernel` solves the batch pairs through
        torch autograd; one without it takes the diagonal of its Gram launch.  lengths_X / lengths_Y: as `compute_Gram`'s; the
        pairs then run on the paired route whatever the shape."""
        assert X.shape[0] == Y.shape[0], "compute_kernel pairs X_i with Y_i"
        if self.normalize:
            return self._normalized_kernel(X, Y, lengths_X, lengths_Y)
        if lengths_X is not None or lengths_Y is not None:
            return self._lengths_kernel(X, Y, lengths_X, lengths_Y)
        static_kind, inv_h = _resolve_static(self.static_kernel, X, Y)
        if static_kind is None and hasattr(self.static_kernel, "batch_kernel"):
            G = self.static_kernel.batch_kernel(X, Y)
            return ops.PDESolve.apply(G, self.dyadic_order, self._naive_solver, *_exact_kw(self.exact_grad).values())
        sigma = None if static_kind is None else _learned_sigma(self.static_kernel)
        if sigma is not None:  # the paired bandwidth launch, whatever the shape
            if not ops.pair_h_takes(X.shape[0], X.shape[1], Y.shape[1], X.shape[2], self.dyadic_order, static_kind,
                                    self._naive_solver, **_exact_kw(self.exact_grad)):
                raise _refused("compute_kernel", X, Y, self.dyadic_order)
            return _SigKernelPairSigma.apply(X, Y, sigma, static_kind, inv_h, self.dyadic_order, self._naive_solver,
                                             *_exact_kw(self.exact_grad).values())
        if static_kind is not None:
            want_grad = torch.is_grad_enabled() and (X.requires_grad or Y.requires_grad)
            if want_grad and self.exact_grad:  # the paired route with the flag, whatever the shape
                if not ops.pair_takes(X.shape[0], X.shape[1], Y.shape[1], X.shape[2], self.dyadic_order, static_kind, True,
                                      exact_adjoint=True):
                    raise _refused("compute_kernel", X, Y, self.dyadic_order, "the exact gradient (exact_grad=True)")
                return _SigKernelPair.apply(X, Y, static_kind, inv_h, self.dyadic_order, self._naive_solver, True)
            if _pair_route(X.shape[0], X.shape[1], Y.shape[1], X.shape[2], static_kind, self.dyadic_order, want_grad,
                           self._naive_solver, _device_cus(X), self.fp32_sweeps):
                return _SigKernelPair.apply(X, Y, static_kind, inv_h, self.dyadic_order, self._naive_solver)
        return self.compute_Gram(X, Y).diagonal()

    def compute_distance(self, X: torch.Tensor, Y: torch.Tensor, lengths_X=None, lengths_Y=None) -> torch.Tensor:
        """mean_i k(X_i, X_i) + mean_i k(Y_i, Y_i) - 2 mean_i k(X_i, Y_i).  lengths_X / lengths_Y: as `compute_Gram`'s."""
        if self.normalize:
            self._log_static("compute_distance", X, Y, lengths_X, lengths_Y)
        if lengths_X is None and lengths_Y is None:
            return (self.compute_kernel(X, X).mean() + self.compute_kernel(Y, Y).mean()
                    - 2.0 * self.compute_kernel(X, Y).mean())
        return (self.compute_kernel(X, X, lengths_X, lengths_X).mean() + self.compute_kernel(Y, Y, lengths_Y, lengths_Y).mean()
                - 2.0 * self.compute_kernel(X, Y, lengths_X, lengths_Y).mean())

    def compute_mmd(self, X: torch.Tensor, Y: torch.Tensor, grad_Y: bool = False, lengths_X=None,
                    lengths_Y=None) -> torch.Tensor:
        """Biased squared MMD: mean K_XX + mean K_YY - 2 mean K_XY.  grad_Y=True differentiates Y through the cross term
        too (`compute_Gram(X, Y, grad_Y=True)`); the default gives Y the gradient of mean K_YY alone.  lengths_X /
        lengths_Y: as `compute_Gram`'s."""
        if self.normalize and self.normalize_route == "fused":  # (its refusals before the first of the three launches)
            self._fused_norm_static("compute_mmd", X, Y, False, False, grad_Y, lengths_X, lengths_Y)
        elif self.normalize:
            self._log_static("compute_mmd", X, Y, lengths_X, lengths_Y)
        if lengths_X is None and lengths_Y is None:
            K_XX = self.compute_Gram(X, X, sym=True)
            K_YY = self.compute_Gram(Y, Y, sym=True)
            K_XY = self.compute_Gram(X, Y, sym=False, grad_Y=grad_Y)
        else:
            K_XX = self.compute_Gram(X, X, sym=True, lengths_X=lengths_X, lengths_Y=lengths_X)
            K_YY = self.compute_Gram(Y, Y, sym=True, lengths_X=lengths_Y, lengths_Y=lengths_Y)
            K_XY = self.compute_Gram(X, Y, sym=False, grad_Y=grad_Y, lengths_X=lengths_X, lengths_Y=lengths_Y)
        return K_XX.mean() + K_YY.mean() - 2.0 * K_XY.mean()

    def gram_and_grad(self, X: torch.Tensor, Y: Optional[torch.Tensor] = None, grad_out=None, sym: bool = False):
        """One fused launch: (K, d sum(grad_out*K)/dX) with detached tensors.  Equivalent to
        `K = compute_Gram(X, Y); g = autograd.grad((grad_out*K).sum(), X)` (score.py:68-69)."""
        Yv = X if Y is None else Y
        if self.normalize and self.normalize_route == "fused":
            static_kind, inv_h = self._fused_norm_static("gram_and_grad", X, Yv, sym, Y is None)
            go = None if grad_out is None else grad_out.detach()
            return ops.gram_fwd_bwd(X, Yv, inv_h, self.dyadic_order, static_kind, go, sym=bool(sym), y_is_x=Y is None,
                                    normalized=True, **_fp32_kw(self.fp32_sweeps))
        if self.normalize:
            return self._normalized_gram_and_grad(X, Yv, grad_out, sym, Y is None)
        static_kind, inv_h = _resolve_static(self.static_kernel, X, Yv)
        if static_kind is None:
            return self._user_gram_and_grad(X, Yv, grad_out, sym)
        cfg = (static_kind, inv_h, self.dyadic_order, self._naive_solver, sym, Y is None, self.fp32_sweeps, self.exact_grad)
        return _solve_gram(X, Yv, cfg, grad_out, True, False, True)[:2]

    def _normalized_gram_and_grad(self, X, Y, grad_out, sym, y_is_x):
        """gram_and_grad with normalize=True: (K^, d sum(grad_out * K^) / dX, first slot) from one
        launch with SIGSVGD_FLAG_NORMALIZED on the long route, whatever the shape; `_log_static`'s refusals"""
        static_kind, inv_h = self._log_static("gram_and_grad", X, Y)
        if not ops.gram_long2_takes(X.shape[0], Y.shape[0], X.shape[1], Y.shape[1], X.shape[2], self.dyadic_order, static_kind,
                                    True, False, y_is_x, normalized=True):
            raise _refused("gram_and_grad", X, Y, self.dyadic_order, "the normalised kernel")
        go = None if grad_out is None else grad_out.detach()
        return ops.gram_long_fwd_bwd2(X, Y, inv_h, self.dyadic_order, static_kind, go, False, bool(sym), y_is_x, True, False,
                                      normalized=True)[:2]

    def _fused_norm_static(self, what, X, Y, sym, y_is_x, grad_Y=False, lengths_X=None, lengths_Y=None):
        """-> (static_kind, inv_h) of a call on the fused route's normalised launch (normalize_route="fused", DESIGN.md section
        5.23), and its refusals, each before any device work"""
        if grad_Y:
            raise NotImplementedError(f"{what}: grad_Y=True with normalize_route='fused': the fused route has the first-slot "
                                      "gradient only; normalize_route='long' returns both")
        if lengths_X is not None or lengths_Y is not None:
            raise NotImplementedError(f"{what}: lengths_X / lengths_Y with normalize_route='fused': the fused route takes one "
                                      "length for every path")
        if _learned_sigma(self.static_kernel) is not None:
            raise NotImplementedError(f"{what}: a static-kernel sigma that requires grad: the bandwidth launches do not take "
                                      "SIGSVGD_FLAG_NORMALIZED_FUSED")
        static_kind, inv_h = _resolve_static(self.static_kernel, X, Y)
        if static_kind is None:
            raise NotImplementedError(f"{what}: the user static kernel {type(self.static_kernel).__name__} runs on "
                                      "ops.PDESolve, which has no normalised form; the built-in static kernels have one")
        if not ops.gram_takes(X.shape[0], Y.shape[0], max(X.shape[1], Y.shape[1]), X.shape[2], self.dyadic_order, static_kind,
                              True, False, bool(sym), bool(y_is_x), normalized=True, **_fp32_kw(self.fp32_sweeps)):
            raise NotImplementedError(f"{what}: {_lib.last_error()}")
        return static_kind, inv_h

    def _user_gram_and_grad(self, X, Y, grad_out, sym):
        """gram_and_grad for a user static kernel: its grid (with the graph to X), K and dG from one PDE launch, and dG
        chained to X through the user's Gram_matrix.  Y is held fixed (first-slot derivative); sym weights grad_out +
        grad_out^T."""
        Xg = X.detach().requires_grad_(True)
        with torch.enable_grad():
            G = self.static_kernel.Gram_matrix(Xg, Y.detach())
        A, B, M, N = G.shape
        go = None if grad_out is None else grad_out.detach().to(G.dtype)
        if sym:
            go = torch.full((A, B), 2.0, dtype=G.dtype, device=G.device) if go is None else go + go.T
        K, dG = ops.pde_fwd_bwd(G.detach().reshape(A * B, M, N), self.dyadic_order, go, self._naive_solver,
                                **_exact_kw(self.exact_grad))
        (gX,) = torch.autograd.grad(G, Xg, dG.reshape(A, B, M, N))
        return K.reshape(A, B), gX


def gram_and_grad(kernel: SigKernel, X, Y=None, grad_out=None):
    return kernel.gram_and_grad(X, Y, grad_out)
