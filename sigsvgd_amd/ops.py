"""Thin torch-facing wrappers over the C ABI (the ONLY place the package touches the HIP library).

Every function takes/returns torch tensors living on an MI355X (`device.type == "cuda"` on ROCm),
checks dtype/contiguity, passes raw device pointers + the current HIP stream to the library and
converts status codes into RuntimeError.  CPU tensors are rejected: there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import torch

from . import _lib

_WS = {}  # (device index, stream) -> uint8 workspace tensor (never needs zeroing: partial sums are stored, not accumulated)


def _require_gpu(*tensors) -> torch.device:
    dev = None
    for t in tensors:
        if t is None:
            continue
        if t.device.type != "cuda":
            raise RuntimeError(
                "sigsvgd_amd: the signature-kernel/SVGD hot path runs only on a HIP device (MI355X); "
                f"got a tensor on '{t.device}'. There is no CPU fallback."
            )
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError(f"sigsvgd_amd: tensors on different devices ({dev} vs {t.device})")
    return dev


def _stream_ptr(dev: torch.device) -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _workspace(dev: torch.device, nbytes: int) -> Tuple[Optional[torch.Tensor], int]:
    if nbytes == 0:
        return None, 0
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
    ws = _WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(int(nbytes * 1.25) + 4096, dtype=torch.uint8, device=dev)
        _WS[key] = ws
    return ws, ws.numel()


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _query(query: str, args, outs, may_refuse: bool = False) -> bool:
    """Host-only query `sigsvgd_<query>(*args, &out...)`.  -> True; False where the library reports SIGSVGD_E_UNSUPPORTED
    and the caller asked whether it takes the launch (`may_refuse`, the `*_takes` predicates); any other error raises."""
    rc = getattr(_lib.load(), "sigsvgd_" + query)(*args, *map(ctypes.byref, outs))
    if may_refuse and rc == _lib.E_UNSUPPORTED:
        return False
    _lib.check(rc, query)
    return True


def _launch(dev: torch.device, name: str, args, query: Optional[str] = None, qargs=()) -> None:
    """The call protocol of every entry point that enqueues work: `sigsvgd_<name>(*args, [workspace, workspace bytes,]
    stream)` on `dev` and its current stream, status turned into RuntimeError.  `query`: the entry point's
    `*_workspace_bytes` query, asked with `qargs`; the workspace is the cached one of (device, stream)."""
    L = _lib.load()
    if query is not None:
        nbytes = ctypes.c_size_t(0)
        _query(query, qargs, (nbytes,))
        ws, wsn = _workspace(dev, nbytes.value)
        args = (*args, _ptr(ws), wsn)
    with torch.cuda.device(dev):
        rc = getattr(L, "sigsvgd_" + name)(*args, _stream_ptr(dev))
    _lib.check(rc, name)


def _weights(grad_out: Optional[torch.Tensor], shape, dtype) -> Optional[torch.Tensor]:
    """grad_out as the library reads it: None (unit weights), or detached, `dtype`, contiguous -- of exactly `shape`, since
    the kernels index it by the launch's own sizes"""
    if grad_out is None:
        return None
    if tuple(grad_out.shape) != tuple(shape):
        raise ValueError(f"grad_out must be [{','.join(map(str, shape))}], got {tuple(grad_out.shape)}")
    return grad_out.detach().to(dtype).contiguous()


def _io_dtype(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return _lib.F32
    if t.dtype == torch.float64:
        return _lib.F64
    raise TypeError(f"sigsvgd_amd: paths must be float32 or float64, got {t.dtype}")


def pad_to_length(P: torch.Tensor, T: int) -> torch.Tensor:
    """[batch, t, d] -> [batch, T, d] with the LAST point repeated.  Exact for the signature kernel: the repeated points add
    zero increments, for which the Goursat stencil copies the solution along the added rows / columns (in every kernel of
    the library: the 4-corner increment of two equal rows of the static kernel is an exact zero), at any dyadic order."""
    t = P.shape[1]
    if t == T:
        return P
    return torch.cat([P, P[:, -1:, :].expand(-1, T - t, -1)], dim=1)


def fold_padded_grad(g: torch.Tensor, t: int) -> torch.Tensor:
    """gradient w.r.t. a path padded by pad_to_length -> gradient w.r.t. the path itself: the copies of the last point add up"""
    if g.shape[1] == t:
        return g
    out = g[:, :t].clone()
    out[:, t - 1] += g[:, t:].sum(dim=1)
    return out


def _prep_paths(X: torch.Tensor, Y: torch.Tensor):
    """-> (X, Y) contiguous, detached, of one dtype and ONE length: upstream sigkernel takes paths of different lengths
    (no caller in the reference does, src/kernels/_traj_kernels.py:200); the shorter batch is padded with its last point,
    which leaves every K[i, j] unchanged (pad_to_length).  The callers fold the gradient back (fold_padded_grad)."""
    if X.dim() != 3 or Y.dim() != 3:
        raise ValueError(f"paths must be [batch, length, dim]; got {tuple(X.shape)} and {tuple(Y.shape)}")
    if X.shape[2] != Y.shape[2]:
        raise ValueError(f"X and Y must share the path dimension (got {tuple(X.shape)} vs {tuple(Y.shape)})")
    if X.dtype != Y.dtype:
        Y = Y.to(X.dtype)
    if X.shape[0] == 0 or Y.shape[0] == 0:
        raise ValueError("empty batch")
    if X.shape[1] < 2 or Y.shape[1] < 2:
        raise ValueError("paths need at least 2 points")
    T = max(X.shape[1], Y.shape[1])
    return pad_to_length(X.detach(), T).contiguous(), pad_to_length(Y.detach(), T).contiguous()


# the settings of a launch, by the names the wrappers give them, as the bits of include/sigsvgd_hip.h
_FLAG_BITS = {"naive": _lib.FLAG_NAIVE_SOLVER, "sym": _lib.FLAG_SYM, "y_is_x": _lib.FLAG_Y_IS_X,
              "force_generic": _lib.FLAG_FORCE_GENERIC, "stored_forward": _lib.FLAG_STORED_FORWARD,
              "fp32_sweeps": _lib.FLAG_FP32_SWEEPS, "exact_adjoint": _lib.FLAG_EXACT_ADJOINT, "nan_tails": _lib.FLAG_NAN_TAILS,
              "log_k": _lib.FLAG_LOG_K, "normalized": _lib.FLAG_NORMALIZED, "normalized_fused": _lib.FLAG_NORMALIZED_FUSED,
              "fold": _lib.FLAG_FOLD_TILES}


def _flags(*in_table_order, **named) -> int:
    """The flag word of the settings that are true, by their names in `_FLAG_BITS`; a name it does not hold is a TypeError.
    This package passes names only; values without one are read in the table's order, as the per-flag tests of tests/ state
    the bits of earlier versions."""
    if len(in_table_order) > len(_FLAG_BITS) or not named.keys() <= _FLAG_BITS.keys() - list(_FLAG_BITS)[:len(in_table_order)]:
        raise TypeError(f"_flags takes {', '.join(_FLAG_BITS)}, each once; got {len(in_table_order)} values and {sorted(named)}")
    named.update(zip(_FLAG_BITS, in_table_order))
    return sum(_FLAG_BITS[name] for name, on in named.items() if on)


def gram_fwd(X, Y, inv_h: float, dyadic_order: int = 0, static_kind: int = _lib.STATIC_RBF,
             naive: bool = False, force_generic: bool = False, y_is_x: bool = False,
             stored_forward: bool = False, fp32_sweeps: bool = False, normalized: bool = False) -> torch.Tensor:
    """K[A,B] = signature-kernel Gram matrix (forward only).  y_is_x: the caller states that Y holds the
    same values as X, so each unordered pair is solved once and K is mirrored.  fp32_sweeps, normalized: see `gram_fwd_bwd`."""
    dev = _require_gpu(X, Y)
    Xc, Yc = _prep_paths(X, Y)
    A, T, d = Xc.shape
    B = Yc.shape[0]
    if y_is_x and X.shape[1] != Y.shape[1]:
        raise ValueError("y_is_x needs X and Y of one shape")
    flags = _flags(naive=naive, y_is_x=bool(y_is_x) and A == B, force_generic=force_generic, stored_forward=stored_forward,
                   fp32_sweeps=fp32_sweeps, normalized_fused=normalized)
    K = torch.empty((A, B), dtype=Xc.dtype, device=dev)
    _launch(dev, "gram_fwd", (Xc.data_ptr(), Yc.data_ptr(), A, B, T, d, _io_dtype(Xc), float(inv_h), int(dyadic_order),
                              int(static_kind), flags, K.data_ptr()),
            "gram_workspace_bytes", (A, B, T, d, int(dyadic_order), int(static_kind), 0, flags))
    return K


def gram_fwd_bwd(X, Y, inv_h: float, dyadic_order: int = 0, static_kind: int = _lib.STATIC_RBF,
                 grad_out: Optional[torch.Tensor] = None, naive: bool = False, sym: bool = False,
                 y_is_x: bool = False, force_generic: bool = False,
                 check_regime: bool = True, stored_forward: bool = False,
                 fp32_sweeps: bool = False, normalized: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """(K[A,B], gradX[A,T,d]) with gradX = d sum(grad_out*K)/dX (first slot); grad_out None = ones.

    `normalized=True` (SIGSVGD_FLAG_NORMALIZED_FUSED; here, on `gram_fwd` and `gram_takes`): K is the
    normalised kernel K^_ij = K(X_i, Y_j) / sqrt(K(X_i, X_i) K(Y_j, Y_j)) and gradX the first-slot gradient of
    sum(grad_out * K^), the diagonals' dependence included -- the unflagged launch of the same route between a diagonal pass
    and two small kernels, one capturable call.  With y_is_x K^'s diagonal is exactly 1 and the diagonal pairs carry no
    gradient.  Defined where K(x, x) fits the dtype (T <= 128 does); `gram_long_fwd_bwd2(normalized=True)` past that.  Not
    with naive.

    Bit-reproducible: every reduction over pairs runs in an order fixed by the launch geometry (no floating-point
    atomics), so two calls on the same input -- eager or replayed from a captured graph -- return the same bits.

    Accuracy (include/sigsvgd_hip.h): every entry of K within 1e-5 of the fp64 reference's, plain |K - K_ref| / |K_ref| --
    the fp32-sweep kernels check every pair for cancellation and for its conditioning in the increments and hand the pairs
    that fail to an exact fp64 pass inside the same call; the gradient of such a pair keeps the fp32 solution (its error is
    relative to the largest gradient entry of the launch).  The exact pass enforces the bound for paths in d <= 4 channels on
    the register-resident kernel (T <= 64) and d <= 3 on the quadrant, refined-grid and band kernels; for d >= 5 it is
    measured, not enforced.  `gram_fwd` and `gram_fwd_bwd` test the conditioning differently (a bound of 300 forward-only,
    the condition number against 150 with the gradient: csrc/sweep_scaffold.h), so the two may return different bits,
    both inside the bound, for a flagged pair.  `force_generic=True`: fp64 sweeps for K and the gradient alike.
    `fp32_sweeps=True` (SIGSVGD_FLAG_FP32_SWEEPS): the IMQ and rational-quadratic static kernels
    (`static_kind` 2, 3), which by default run on the fp64 coverage kernel and are held to fp64 results, take the
    register-resident fp32-sweep kernel RBF runs at dyadic order 0, 3 <= T <= 64, d <= 16 -- and with it the accuracy above
    (K per entry within 1e-5, the gradient within 1e-5 of its largest entry).  One-channel gradient launches stay on the
    coverage kernel as for RBF.  RBF paths of 17 <= d <= 32 channels at order 0, 3 <= T <= 64, which by
    default run on the coverage kernel, take the same kernel's 32-channel layout at the same accuracy.  For every other kind,
    shape, order or solver the argument changes nothing.
    `check_regime` and `stored_forward` are accepted for callers written against earlier versions (when long paths
    could run on a kernel that regenerated the forward solution and declined rough pairs) and have no effect."""
    dev = _require_gpu(X, Y, grad_out)
    Xc, Yc = _prep_paths(X, Y)
    A, T, d = Xc.shape
    B = Yc.shape[0]
    go = _weights(grad_out, (A, B), Xc.dtype)
    if (y_is_x or sym) and X.shape[1] != Y.shape[1]:
        raise ValueError("y_is_x / sym need X and Y of one shape")
    flags = _flags(naive=naive, sym=sym, y_is_x=y_is_x, force_generic=force_generic, stored_forward=stored_forward,
                   fp32_sweeps=fp32_sweeps, normalized_fused=normalized)
    K = torch.empty((A, B), dtype=Xc.dtype, device=dev)
    gX = torch.empty((A, T, d), dtype=Xc.dtype, device=dev)
    _launch(dev, "gram_fwd_bwd", (Xc.data_ptr(), Yc.data_ptr(), A, B, T, d, _io_dtype(Xc), float(inv_h), int(dyadic_order),
                                  int(static_kind), flags, _ptr(go), K.data_ptr(), gX.data_ptr()),
            "gram_workspace_bytes", (A, B, T, d, int(dyadic_order), int(static_kind), 1, flags))
    return K, fold_padded_grad(gX, X.shape[1])


def gram_takes(A: int, B: int, T: int, d: int, dyadic_order: int = 0, static_kind: int = _lib.STATIC_RBF,
               want_grad: bool = True, naive: bool = False, sym: bool = False, y_is_x: bool = False,
               fp32_sweeps: bool = False, normalized: bool = False) -> bool:
    """Whether `gram_fwd` (want_grad False) / `gram_fwd_bwd` take paths [A, T, d] x [B, T, d] with these settings: the
    library's workspace query for the call's flags, host only.  False exactly where it reports SIGSVGD_E_UNSUPPORTED (the
    per-pair state outgrows the LDS: the long route, `gram_long_fwd*`, takes those; normalized together with naive, or a
    shape whose diagonal pass the paired plan refuses); any other error raises."""
    flags = _flags(naive=naive, sym=sym and want_grad, y_is_x=bool(y_is_x) and (want_grad or A == B), fp32_sweeps=fp32_sweeps,
                   normalized_fused=normalized)
    return _query("gram_workspace_bytes", (int(A), int(B), int(T), int(d), int(dyadic_order), int(static_kind),
                                           1 if want_grad else 0, flags), (ctypes.c_size_t(0),), may_refuse=True)


def _prep_long(X, Y):
    """-> (X, Y) contiguous, detached, of X's dtype, each at its own length (the long route takes TX != TY)."""
    if X.dim() != 3 or Y.dim() != 3:
        raise ValueError(f"paths must be [batch, length, dim]; got {tuple(X.shape)} and {tuple(Y.shape)}")
    if X.shape[2] != Y.shape[2]:
        raise ValueError(f"X and Y must share the path dimension (got {tuple(X.shape)} vs {tuple(Y.shape)})")
    if X.shape[0] == 0 or Y.shape[0] == 0:
        raise ValueError("empty batch")
    if X.shape[1] < 2 or Y.shape[1] < 2:
        raise ValueError("paths need at least 2 points")
    _io_dtype(X)
    return X.detach().contiguous(), Y.detach().to(X.dtype).contiguous()


def _prep_pair(X, Y):
    if X.dim() != 3 or Y.dim() != 3 or X.shape[0] != Y.shape[0]:
        raise ValueError(f"pairs need X [A, TX, d] and Y [A, TY, d]; got {tuple(X.shape)} and {tuple(Y.shape)}")
    return _prep_long(X, Y)


# ---- the long route: what its seven launches and their queries share -------------------------------------------------------------
def _long_geometry(pair: bool, A, B, TX, TY, d, dyadic_order, static_kind, wants, flags: int):
    """-> (shape, query arguments) of a long-route call, the one place that knows their order (`_lib.ARGTYPES`): the shape is
    A, B, TX, TY, d in the Gram mode and A, TX, TY, d in the paired one; a launch states X, Y, shape, dtype, inv_h, order,
    kind, flags, its query shape, order, kind, `wants` as 0 / 1, flags."""
    shape = (int(A), int(TX), int(TY), int(d)) if pair else (int(A), int(B), int(TX), int(TY), int(d))
    return shape, (*shape, int(dyadic_order), int(static_kind), *(1 if w else 0 for w in wants), flags)


def _long_query(query: str, pair: bool, A, B, TX, TY, d, dyadic_order, static_kind, wants, outs=None, **settings) -> bool:
    """A host-only query of the long route: `_query` with the arguments of `_long_geometry`; without `outs` the `*_takes`
    question (False exactly where the library reports SIGSVGD_E_UNSUPPORTED)."""
    _, qargs = _long_geometry(pair, A, B, TX, TY, d, dyadic_order, static_kind, wants, _flags(**settings))
    return _query(query, qargs, outs or (ctypes.c_size_t(0),), may_refuse=outs is None)


def _long_launch(name: str, query: str, X, Y, inv_h, dyadic_order, static_kind, wants, pair: bool = False, weights=(),
                 grads=(), with_dK: bool = False, **settings):
    """A launch of the long route, -> (K, the gradient of each slot in `grads` or None, dK_dinvh if `with_dK`): the paths
    prepared, K [A, B] (`pair`: [A]) and the outputs allocated in X's dtype, `sigsvgd_<name>` launched with the workspace of
    `sigsvgd_<query>(..., *wants, flags)`.  weights: (grad_out,) where the entry point has the argument; grads: one want per
    gradient output the entry point has (X's, then Y's); settings: the keywords of `_flags`."""
    dev = _require_gpu(X, Y, *weights)
    Xc, Yc = (_prep_pair if pair else _prep_long)(X, Y)
    (A, TX, d), (B, TY) = Xc.shape, Yc.shape[:2]
    if (settings.get("sym") or settings.get("y_is_x")) and (A != B or TX != TY):
        raise ValueError("sym and y_is_x need X and Y of one shape")
    flags = _flags(**settings)
    shape, qargs = _long_geometry(pair, A, B, TX, TY, d, dyadic_order, static_kind, wants, flags)
    new = lambda *size: torch.empty(size, dtype=Xc.dtype, device=dev)
    outs = [new(*shape[:1 if pair else 2])]
    go = [_weights(w, outs[0].shape, Xc.dtype) for w in weights]
    outs += [new(*size) if want else None for want, size in zip(grads, ((A, TX, d), (B, TY, d)))]
    if with_dK:
        outs.append(new(*outs[0].shape))
    _launch(dev, name, (Xc.data_ptr(), Yc.data_ptr(), *shape, _io_dtype(Xc), float(inv_h), int(dyadic_order), int(static_kind),
                        flags, *map(_ptr, go + outs)), query, qargs)
    return tuple(outs)


def gram_long_fwd(X, Y, inv_h: float, dyadic_order: int = 0, static_kind: int = _lib.STATIC_RBF,
                  naive: bool = False) -> torch.Tensor:
    """K[A,B] of the built-in static kernels on long paths (`sigsvgd_gram_long_fwd`, csrc/gram_long.hip): the launches
    `gram_fwd` refuses for LDS.  X [A,TX,d] and Y [B,TY,d] at their own lengths; fp64 increments and sweeps, K in X's
    dtype."""
    return _long_launch("gram_long_fwd", "gram_long_workspace_bytes", X, Y, inv_h, dyadic_order, static_kind, (0,),
                        naive=naive)[0]


def gram_long_fwd_bwd(X, Y, inv_h: float, dyadic_order: int = 0, static_kind: int = _lib.STATIC_RBF,
                      grad_out: Optional[torch.Tensor] = None, naive: bool = False,
                      sym: bool = False, exact_adjoint: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """(K[A,B], gradX[A,TX,d]) with gradX = d sum(grad_out*K)/dX (first slot; grad_out None = ones; sym: grad_out +
    grad_out^T) on the long route (`sigsvgd_gram_long_fwd_bwd`).  Bit-reproducible.  Every ordered pair is solved, also
    when Y holds X's values, and Y gets no gradient: `gram_long_fwd_bwd2` solves Y = X once per unordered pair and returns
    the gradients of both slots.  exact_adjoint (SIGSVGD_FLAG_EXACT_ADJOINT; here and on every
    gradient launch of the long route below): gX is the exact derivative of the discrete K returned -- the adjoint of the
    default stencil itself -- instead of the reference's GG convention, which differs from it by per cents; K has the
    same bits, the workspace the same bytes.  With naive=True (where GG is exact) it changes nothing."""
    return _long_launch("gram_long_fwd_bwd", "gram_long_workspace_bytes", X, Y, inv_h, dyadic_order, static_kind, (1,),
                        weights=(grad_out,), grads=(True,), naive=naive, sym=sym, exact_adjoint=exact_adjoint)


def gram_long2_takes(A: int, B: int, TX: int, TY: int, d: int, dyadic_order: int = 0, static_kind: int = _lib.STATIC_RBF,
                     want_gradX: bool = True, want_gradY: bool = True, y_is_x: bool = False,
                     exact_adjoint: bool = False, nan_tails: bool = False, log_k: bool = False,
                     normalized: bool = False) -> bool:
    """Whether `gram_long_fwd_bwd2` takes paths X [A, TX, d] x Y [B, TY, d] with these outputs: the library's workspace
    query, host only.  False exactly where it reports SIGSVGD_E_UNSUPPORTED (past 8192 refined cells on a side, or per-wave
    state beyond the LDS; nan_tails together with exact_adjoint; log_k together with either; normalized together with any of
    the three); any other error raises."""
    return _long_query("gram_long2_workspace_bytes", False, A, B, TX, TY, d, dyadic_order, static_kind,
                       (want_gradX, want_gradY), y_is_x=y_is_x, exact_adjoint=exact_adjoint, nan_tails=nan_tails, log_k=log_k,
                       normalized=normalized)


def gram_long_fwd_bwd2(X, Y, inv_h: float, dyadic_order: int = 0, static_kind: int = _lib.STATIC_RBF,
                       grad_out: Optional[torch.Tensor] = None, naive: bool = False, sym: bool = False,
                       y_is_x: bool = False, want_gradX: bool = True, want_gradY: bool = True,
                       exact_adjoint: bool = False, nan_tails: bool = False, log_k: bool = False,
                       normalized: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor]]:
    """(K[A,B], gX[A,TX,d] or None, gY[B,TY,d] or None) on the long route from one solve per pair
    (`sigsvgd_gram_long_fwd_bwd2`): gX = d sum(grad_out*K)/dX and gY = d sum(grad_out*K)/dY, each its own slot (grad_out
    None = ones), K bit-identical to `gram_long_fwd`.  y_is_x (Y holds X's values; A == B, TX == TY): each unordered pair is
    solved once, K's lower triangle mirrors the upper one, and gX is the first-slot gradient `gram_long_fwd_bwd` returns;
    sym: weights grad_out + grad_out^T.  Both give no gY (it is returned as None).  Neither gradient wanted: forward only.
    Computed and returned in X's dtype; bit-reproducible.  nan_tails (SIGSVGD_FLAG_NAN_TAILS; here
    and on the paired launches below): a path ends before its first point whose channel 0 is NaN, pair (i, j) is solved on
    its own grid, and the gradient rows from a path's end on are exact zeros.  log_k (SIGSVGD_FLAG_LOG_K, DESIGN.md section
    5.21; here and on the paired launches below): the first result is ln K and the gradients are those of sum(grad_out * ln K),
    from sweeps that carry a running power-of-two scale, so nothing overflows while ln K itself is representable; a pair
    whose discrete K is <= 0 gives NaN.  Default stencil only, not with exact_adjoint or nan_tails.  normalized
    (SIGSVGD_FLAG_NORMALIZED; this launch only): the first result is the normalised kernel
    K^_ij = K(X_i, Y_j) / sqrt(K(X_i, X_i) K(Y_j, Y_j)), formed in the log domain, and the gradients are those of
    sum(grad_out * K^), the diagonals' dependence included, each slot its own; with y_is_x gX is the gradient in X_i of
    sum_j grad_out_ij K^(X_i, Y_j) at fixed Y = X (SVGD's), and K^'s diagonal is exactly 1.  Every pair is solved once.  Not
    with naive, exact_adjoint, nan_tails or log_k."""
    wants = (want_gradX, bool(want_gradY) and not (sym or y_is_x))
    return _long_launch("gram_long_fwd_bwd2", "gram_long2_workspace_bytes", X, Y, inv_h, dyadic_order, static_kind, wants,
                        weights=(grad_out,), grads=wants, naive=naive, sym=sym, y_is_x=y_is_x, exact_adjoint=exact_adjoint,
                        nan_tails=nan_tails, log_k=log_k, normalized=normalized)


def pair_takes(A: int, TX: int, TY: int, d: int, dyadic_order: int = 0, static_kind: int = _lib.STATIC_RBF,
               want_grad: bool = True, exact_adjoint: bool = False, nan_tails: bool = False, log_k: bool = False) -> bool:
    """Whether `pair_fwd` (want_grad False) / `pair_fwd_bwd` take pairs X [A, TX, d], Y [A, TY, d]: the library's workspace
    query, host only.  False exactly where it reports SIGSVGD_E_UNSUPPORTED (past 8192 refined cells on a side, or per-wave
    state beyond the LDS; nan_tails together with exact_adjoint; log_k together with either); any other error raises."""
    return _long_query("pair_workspace_bytes", True, A, A, TX, TY, d, dyadic_order, static_kind, (want_grad,),
                       exact_adjoint=exact_adjoint, nan_tails=nan_tails, log_k=log_k)


def pair_schedule(A: int, TX: int, TY: int, d: int, dyadic_order: int = 0, static_kind: int = _lib.STATIC_RBF,
                  want_grad: bool = True, exact_adjoint: bool = False, nan_tails: bool = False,
                  log_k: bool = False) -> Tuple[int, int, int]:
    """(waves_per_pair, grid, lds_bytes) of the paired launch these arguments would run now (`sigsvgd_pair_schedule`, host
    only, SIGSVGD_PAIR_MODE included): 1 wave per pair is the serial kernel of csrc/gram_long.hip, more the band-parallel one
    of csrc/pair_bands.hip.  The results do not depend on it, bit for bit.  exact_adjoint: gradient launches with it always
    run 1 wave per pair, and so does every launch with nan_tails or log_k."""
    waves, grid, lds = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_size_t(0)
    _long_query("pair_schedule", True, A, A, TX, TY, d, dyadic_order, static_kind, (want_grad,), (waves, grid, lds),
                exact_adjoint=exact_adjoint, nan_tails=nan_tails, log_k=log_k)
    return waves.value, grid.value, lds.value


def pair_fwd(X, Y, inv_h: float, dyadic_order: int = 0, static_kind: int = _lib.STATIC_RBF,
             naive: bool = False, nan_tails: bool = False, log_k: bool = False) -> torch.Tensor:
    """K[A] = k_sig(X_i, Y_i) of the built-in static kernels (`sigsvgd_pair_fwd`, the paired mode of csrc/gram_long.hip): one
    solve per pair.  X [A,TX,d] and Y [A,TY,d] at their own lengths; fp64 increments and sweeps, K in X's dtype, bit-identical
    to the diagonal of `gram_long_fwd(X, Y)`.  log_k: ln K, bit-identical to the diagonal of the two-sided launch with log_k."""
    return _long_launch("pair_fwd", "pair_workspace_bytes", X, Y, inv_h, dyadic_order, static_kind, (0,), pair=True,
                        naive=naive, nan_tails=nan_tails, log_k=log_k)[0]


def pair_fwd_bwd(X, Y, inv_h: float, dyadic_order: int = 0, static_kind: int = _lib.STATIC_RBF,
                 grad_out: Optional[torch.Tensor] = None, naive: bool = False, want_x: bool = True, want_y: bool = True,
                 exact_adjoint: bool = False, nan_tails: bool = False,
                 log_k: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor]]:
    """(K[A], gX[A,TX,d] or None, gY[A,TY,d] or None): gX = d sum(grad_out*K)/dX and gY = d sum(grad_out*K)/dY, each path's
    own slot (grad_out None = ones), from one forward and one reverse sweep per pair (`sigsvgd_pair_fwd_bwd`).  Computed
    and returned in X's dtype; bit-reproducible."""
    if not (want_x or want_y):
        raise ValueError("pair_fwd_bwd needs want_x or want_y (pair_fwd for the forward only)")
    return _long_launch("pair_fwd_bwd", "pair_workspace_bytes", X, Y, inv_h, dyadic_order, static_kind, (1,), pair=True,
                        weights=(grad_out,), grads=(want_x, want_y), naive=naive, exact_adjoint=exact_adjoint,
                        nan_tails=nan_tails, log_k=log_k)


def gram_long_h_takes(A: int, B: int, TX: int, TY: int, d: int, dyadic_order: int = 0, static_kind: int = _lib.STATIC_RBF,
                      want_gradX: bool = True, want_gradY: bool = True, naive: bool = False, y_is_x: bool = False,
                      exact_adjoint: bool = False) -> bool:
    """Whether `gram_long_fwd_bwd_h` takes paths X [A, TX, d] x Y [B, TY, d] with these outputs: the library's workspace
    query, host only.  False exactly where it reports SIGSVGD_E_UNSUPPORTED (past 8192 refined cells on a side, per-wave
    state beyond the LDS, or the first-order stencil with IMQ / rational quadratic / Matern); any other error raises."""
    return _long_query("gram_long_h_workspace_bytes", False, A, B, TX, TY, d, dyadic_order, static_kind,
                       (want_gradX, want_gradY), naive=naive, y_is_x=y_is_x, exact_adjoint=exact_adjoint)


def gram_long_fwd_bwd_h(X, Y, inv_h: float, dyadic_order: int = 0, static_kind: int = _lib.STATIC_RBF,
                        grad_out: Optional[torch.Tensor] = None, naive: bool = False, sym: bool = False,
                        y_is_x: bool = False, want_gradX: bool = True, want_gradY: bool = True, exact_adjoint: bool = False):
    """(K[A,B], gX or None, gY or None, dK_dinvh[A,B]): `gram_long_fwd_bwd2` with every pair's derivative of K in the
    static kernel's inverse bandwidth from the same reverse sweep (`sigsvgd_gram_long_fwd_bwd_h`, DESIGN.md section 5.16;
    RBF, IMQ, rational quadratic and Matern).  dK_dinvh is unweighted -- grad_out and sym weight gX and gY only -- and with y_is_x
    exactly symmetric; dK/dsigma = -inv_h^2 dK_dinvh.  K, gX and gY have the bits `gram_long_fwd_bwd2` returns.  Neither
    gradient wanted: the reverse sweep still runs.  Bit-reproducible."""
    wants = (want_gradX, bool(want_gradY) and not (sym or y_is_x))
    return _long_launch("gram_long_fwd_bwd_h", "gram_long_h_workspace_bytes", X, Y, inv_h, dyadic_order, static_kind, wants,
                        weights=(grad_out,), grads=wants, with_dK=True, naive=naive, sym=sym, y_is_x=y_is_x,
                        exact_adjoint=exact_adjoint)


def pair_h_takes(A: int, TX: int, TY: int, d: int, dyadic_order: int = 0, static_kind: int = _lib.STATIC_RBF,
                 naive: bool = False, exact_adjoint: bool = False) -> bool:
    """Whether `pair_fwd_bwd_h` takes pairs X [A, TX, d], Y [A, TY, d]: the library's workspace query, host only.  False
    exactly where it reports SIGSVGD_E_UNSUPPORTED (as `gram_long_h_takes`); any other error raises."""
    return _long_query("pair_h_workspace_bytes", True, A, A, TX, TY, d, dyadic_order, static_kind, (), naive=naive,
                       exact_adjoint=exact_adjoint)


def pair_fwd_bwd_h(X, Y, inv_h: float, dyadic_order: int = 0, static_kind: int = _lib.STATIC_RBF,
                   grad_out: Optional[torch.Tensor] = None, naive: bool = False, want_x: bool = True, want_y: bool = True,
                   exact_adjoint: bool = False):
    """(K[A], gX or None, gY or None, dK_dinvh[A]): `pair_fwd_bwd` with each pair's derivative of K in the static kernel's
    inverse bandwidth (`sigsvgd_pair_fwd_bwd_h`), unweighted; equal, bit for bit, to the diagonal of
    `gram_long_fwd_bwd_h`'s.  K, gX and gY have the bits `pair_fwd_bwd` returns; neither gradient wanted is allowed.  Always
    the one-wavefront schedule."""
    return _long_launch("pair_fwd_bwd_h", "pair_h_workspace_bytes", X, Y, inv_h, dyadic_order, static_kind, (), pair=True,
                        weights=(grad_out,), grads=(want_x, want_y), with_dK=True, naive=naive, exact_adjoint=exact_adjoint)


def path_sqdist_select(X, Y: Optional[torch.Tensor] = None, rank: Optional[int] = None) -> torch.Tensor:
    """The element of rank `rank` (zero-based, ascending; default the lower median (n - 1) // 2, what `torch.median` returns)
    of the n = A B TX TY squared distances |X_ip - Y_jq|^2 between the points of X [A,TX,d] and Y [B,TY,d], as a 0-dim fp64
    tensor on the device (`sigsvgd_sqdist_select`, csrc/sqdist_select.hip).  Exact on the fp64 difference-form values; the
    [A,B,TX,TY] tensor is never formed and nothing is read back.  Y None: Y = X, each unordered pair of paths visited once
    (the same result, bit for bit)."""
    dev = _require_gpu(X, Y)
    if X.dim() != 3 or (Y is not None and Y.dim() != 3):
        raise ValueError("paths must be [batch, length, dim]")
    if Y is not None and X.shape[2] != Y.shape[2]:
        raise ValueError(f"X and Y must share the path dimension (got {tuple(X.shape)} vs {tuple(Y.shape)})")
    _io_dtype(X)
    Xc = X.detach().contiguous()
    Yc = Xc if Y is None else Y.detach().to(X.dtype).contiguous()
    if Xc.numel() == 0 or Yc.numel() == 0:
        raise ValueError("empty batch")
    (A, TX, d), (B, TY) = Xc.shape, Yc.shape[:2]
    n = A * B * TX * TY
    rank = (n - 1) // 2 if rank is None else int(rank)
    if not 0 <= rank < n:
        raise ValueError(f"rank {rank} outside the {n} elements")
    flags = _flags(y_is_x=Y is None)
    out = torch.empty((), dtype=torch.float64, device=dev)
    _launch(dev, "sqdist_select", (Xc.data_ptr(), Yc.data_ptr(), A, B, TX, TY, d, _io_dtype(Xc), flags, rank, out.data_ptr()),
            "sqdist_select_workspace_bytes", (A, B, TX, TY, d, flags))
    return out


def path_sqdist_select_passes(dev: torch.device) -> int:
    """How many passes of the last `path_sqdist_select` on this device and stream recomputed the distances (at most 6): the
    counter the select keeps at the start of its workspace (csrc/sqdist_select.hip, SelState).  Synchronises; for
    scripts/median_time.py."""
    ws = _WS[(dev.index, torch.cuda.current_stream(dev).cuda_stream)]
    off = (-ws.data_ptr()) % 256
    return int(ws[off + 28:off + 32].view(torch.int32).item())


def _flat32(t: torch.Tensor, N: int) -> torch.Tensor:
    return t.detach().to(torch.float32).reshape(N, -1).contiguous()


def _update_operands(dev, shape, D: int, X, mask, inplace: bool, adagrad_state, like: str):
    """-> (X, mask) as the update launches read them, each [N, D] fp32 or None, for a velocity of `shape` = [N, ...]: the mask
    broadcast to it, X refused for `inplace` unless it is its own flattening, adagrad_state refused unless the launch can
    add to it where it is.  `like`: what the error text calls the velocity's shape."""
    N = shape[0]
    Xc = None
    if X is not None:
        Xc = _flat32(X, N)
        if inplace and Xc.data_ptr() != X.data_ptr():  # (in place, every element is read and written by the same thread)
            raise ValueError("inplace update needs contiguous float32 particles")
    m = None
    if mask is not None:
        m = torch.broadcast_to(torch.as_tensor(mask, dtype=torch.float32, device=dev), shape).reshape(N, -1).contiguous()
    if adagrad_state is not None and (adagrad_state.dtype != torch.float32 or not adagrad_state.is_contiguous()
                                      or adagrad_state.numel() != N * D):
        raise ValueError(f"adagrad_state must be a contiguous float32 tensor with the shape of {like}")
    return Xc, m


def svgd_phi(K, score, grad_k, mask=None, X=None, lr: Optional[float] = None, adagrad_state=None,
             inplace: bool = False):
    """v = -((K @ score - grad_k)/N) [* mask]; with X and lr also returns X - lr*v.

    All fp32, shapes K [N,N], score/grad_k/mask/X [N, ...] (flattened to [N,D]).
    adagrad_state: contiguous fp32 tensor shaped like score, updated IN PLACE (state += v^2) and applied
    (v / sqrt(state + 1e-12)) before the update -- the reference's adaptive_gradient=True (svgd.py:110-113).
    Returns v (shaped like score) or (v, X_new)."""
    dev = _require_gpu(K, score, grad_k, mask, X, adagrad_state)
    N = K.shape[0]
    if K.dim() != 2 or K.shape[1] != N:
        raise ValueError(f"K must be square, got {tuple(K.shape)}")
    if X is not None and lr is None:
        raise ValueError("lr is required with X")
    shape = score.shape
    Kc = K.detach().to(torch.float32).contiguous()
    s, gk = _flat32(score, N), _flat32(grad_k, N)
    D = s.shape[1]
    if score.shape[0] != N:
        raise ValueError(f"score must have K's {N} rows, got {tuple(score.shape)}")
    if gk.shape != s.shape:
        raise ValueError(f"grad_k shape {tuple(grad_k.shape)} does not match score {tuple(score.shape)}")
    Xc, m = _update_operands(dev, shape, D, X, mask, inplace, adagrad_state, "score")
    if Xc is not None and Xc.shape != s.shape:  # (the kernel indexes X_in and X_out by the launch's N and D)
        raise ValueError(f"X shape {tuple(X.shape)} does not match score {tuple(score.shape)}")
    v = torch.empty_like(s)
    Xn = Xc if inplace or Xc is None else torch.empty_like(Xc)
    _launch(dev, "svgd_step", (Kc.data_ptr(), s.data_ptr(), gk.data_ptr(), _ptr(m), N, D, v.data_ptr(), _ptr(Xc), _ptr(Xn),
                               float(lr or 0.0), _ptr(adagrad_state)))
    v = v.reshape(shape)
    if X is not None:
        return v, (X if inplace else Xn.reshape(X.shape))
    return v


class AdamState:
    """State of the fused Adam update (torch.optim.Adam semantics): exp_avg / exp_avg_sq [N, D] fp32 and the step
    counter, all on the device (the counter too, so a captured graph can replay the update)."""

    def __init__(self, like: torch.Tensor, betas=(0.9, 0.999), eps: float = 1e-8):
        n = like.shape[0]
        self.exp_avg = torch.zeros((n, like.numel() // n), dtype=torch.float32, device=like.device)
        self.exp_avg_sq = torch.zeros_like(self.exp_avg)
        self.step = torch.zeros((), dtype=torch.int32, device=like.device)
        self.t_host = 0  # host mirror of the counter (no read-back needed to export the state)
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)


def svgd_adam(K, score, grad_k, X, lr: float, state: AdamState, mask=None, inplace: bool = False):
    """v = -((K @ score - grad_k)/N) [* mask] and torch.optim.Adam's update of X along it, one launch (plus a
    one-thread launch that advances the device-side step counter).  Returns (v shaped like score, X_new);
    inplace=True writes the update into X itself (X must be contiguous fp32) and returns X."""
    dev = _require_gpu(K, score, grad_k, mask, X, state.exp_avg)
    N = K.shape[0]
    if K.dim() != 2 or K.shape[1] != N:
        raise ValueError(f"K must be square, got {tuple(K.shape)}")
    shape = score.shape
    Kc = K.detach().to(torch.float32).contiguous()
    s, gk = _flat32(score, N), _flat32(grad_k, N)
    D = s.shape[1]
    if score.shape[0] != N:
        raise ValueError(f"score must have K's {N} rows, got {tuple(score.shape)}")
    Xc, m = _update_operands(dev, shape, D, X, mask, inplace, None, "score")
    if gk.shape != s.shape or Xc.shape != s.shape or tuple(state.exp_avg.shape) != (N, D) \
            or tuple(state.exp_avg_sq.shape) != (N, D):
        raise ValueError("score, grad_k, X and the Adam state must share the shape [N, D]")
    v = torch.empty_like(s)
    Xn = Xc if inplace else torch.empty_like(Xc)
    _launch(dev, "svgd_adam_step", (Kc.data_ptr(), s.data_ptr(), gk.data_ptr(), _ptr(m), N, D, v.data_ptr(), Xc.data_ptr(),
                                    Xn.data_ptr(), float(lr), state.betas[0], state.betas[1], state.eps,
                                    state.exp_avg.data_ptr(), state.exp_avg_sq.data_ptr(), state.step.data_ptr()))
    state.t_host += 1
    return v.reshape(shape), (X if inplace else Xn.reshape(X.shape))


def svgd_update(v, X, lr: float, mask=None, adagrad_state=None, adam: Optional[AdamState] = None, inplace: bool = False,
                want_v: bool = True):
    """The update rules of `svgd_phi` / `svgd_adam` on a velocity that is GIVEN: v [N, ...] = -((K @ score - grad_k)/N), what
    `svgd_phi(K, score, grad_k)` returns (`sigsvgd_svgd_update`: one elementwise launch that shares the fused launches' device
    function, so the results have their bits).  The sharded step runs it on its own rows behind the reduce-scatter.

    mask / adagrad_state / inplace as in `svgd_phi`; adam: an `AdamState` shaped like v (then torch.optim.Adam's update
    along the masked velocity, plus the one-thread launch that advances the device counter; not together with
    adagrad_state).  v is left as it was.  Returns (v_applied, X_new): the velocity after mask and Adagrad, shaped like v,
    and the updated particles (X itself with inplace=True).  want_v=False: v_applied is neither allocated nor stored (the
    entry point's v_out == NULL) and None is returned in its place."""
    dev = _require_gpu(v, X, mask, adagrad_state, adam.exp_avg if adam is not None else None)
    if adam is not None and adagrad_state is not None:
        raise ValueError("svgd_update: Adam and Adagrad state together")
    N, shape = v.shape[0], v.shape
    vc = _flat32(v, N)
    D = vc.shape[1]
    Xc, m = _update_operands(dev, shape, D, X, mask, inplace, adagrad_state, "the velocity")
    if Xc.shape != vc.shape:
        raise ValueError(f"X shape {tuple(X.shape)} does not match the velocity {tuple(v.shape)}")
    if adam is not None and (tuple(adam.exp_avg.shape) != (N, D) or tuple(adam.exp_avg_sq.shape) != (N, D)):
        raise ValueError("the velocity, X and the Adam state must share the shape [N, D]")
    Xn = Xc if inplace else torch.empty_like(Xc)
    vo = torch.empty_like(vc) if want_v else None
    if adam is not None:
        moments = (adam.exp_avg.data_ptr(), adam.exp_avg_sq.data_ptr(), adam.step.data_ptr(), *adam.betas, adam.eps)
    else:
        moments = (None, None, None, 0.0, 0.0, 0.0)
    _launch(dev, "svgd_update", (vc.data_ptr(), _ptr(m), N, D, _ptr(vo), Xc.data_ptr(), Xn.data_ptr(), float(lr),
                                 _ptr(adagrad_state), *moments))
    if adam is not None:
        adam.t_host += 1
    return (vo.reshape(shape) if want_v else None), (X if inplace else Xn.reshape(X.shape))


def _partial_out(out, Xc: torch.Tensor, dev: torch.device) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (K_partial [N,N] of X's dtype, zeroed; grad_partial [N,T,d] fp64, which the library overwrites in full) of a
    partial solve on Xc [N,T,d]: the caller's `out` pair if it fits, else new tensors"""
    N, T, d = Xc.shape
    if out is None:
        return torch.zeros((N, N), dtype=Xc.dtype, device=dev), torch.empty((N, T, d), dtype=torch.float64, device=dev)
    Kp, gp = out
    if (tuple(Kp.shape) != (N, N) or Kp.dtype != Xc.dtype or not Kp.is_contiguous() or tuple(gp.shape) != (N, T, d)
            or gp.dtype != torch.float64 or not gp.is_contiguous()):
        raise ValueError("out must be (K_partial [N,N] of X's dtype, grad_partial [N,T,d] float64), contiguous")
    Kp.zero_()
    return Kp, gp


def gram_sym_partial(X, inv_h: float, tile_offset: int, tile_stride: int, static_kind: int = _lib.STATIC_RBF,
                     grad_out: Optional[torch.Tensor] = None, sym: bool = False, out=None, fold: bool = False,
                     fp32_sweeps: bool = False):
    """This rank's share of the symmetric Gram + gradient on the gathered particles X [N,T,d]:
    returns (K_partial [N,N] X.dtype, grad_partial [N,T,d] fp64), zero outside the owned pairs.
    Summed over tile_offset = 0..tile_stride-1 they equal gram_fwd_bwd(X, X, y_is_x=True).
    The launch owns the row tiles (`sym_tile_rows(T, d)` rows each) tile_offset + k*tile_stride; with fold=True also
    their mirror images, which gives every rank the same number of pairs (SIGSVGD_FLAG_FOLD_TILES).
    `out=(K_partial, grad_partial)` reuses the caller's buffers (K_partial is re-zeroed, grad_partial overwritten).
    RBF, or with `fp32_sweeps=True` (see `gram_fwd_bwd`) the IMQ and rational-quadratic kernels at T <= 64."""
    dev = _require_gpu(X, grad_out)
    Xc, _ = _prep_paths(X, X)
    N, T, d = Xc.shape
    go = _weights(grad_out, (N, N), Xc.dtype)
    Kp, gp = _partial_out(out, Xc, dev)
    flags = _flags(sym=sym, y_is_x=True, fp32_sweeps=fp32_sweeps, fold=fold)
    _launch(dev, "gram_sym_partial", (Xc.data_ptr(), N, T, d, _io_dtype(Xc), float(inv_h), int(static_kind), flags,
                                      int(tile_offset), int(tile_stride), _ptr(go), Kp.data_ptr(), gp.data_ptr()),
            "gram_workspace_bytes", (N, N, T, d, 0, int(static_kind), 1, flags))
    return Kp, gp


def _long_partial_plan(N, T, d, dyadic_order, static_kind, tile_stride, may_refuse: bool) -> Optional[Tuple[int, int]]:
    """(R, JC) of `sigsvgd_gram_long_partial_plan`, or None where the library refuses the shape and `may_refuse`"""
    R, JC = ctypes.c_int(0), ctypes.c_int(0)
    if not _query("gram_long_partial_plan", (int(N), int(T), int(d), int(dyadic_order), int(static_kind), 0,
                                             int(tile_stride)), (R, JC), may_refuse):
        return None
    return int(R.value), int(JC.value)


def gram_long_partial_tiles(N: int, T: int, d: int, dyadic_order: int = 0, static_kind: int = _lib.STATIC_RBF,
                            tile_stride: int = 1) -> Tuple[int, int]:
    """(R, JC): rows per owned tile and columns per work item of `gram_long_sym_partial` on N paths [T, d] shared among
    tile_stride ranks (`sigsvgd_gram_long_partial_plan`, host only).  The same for every rank and for folded and cyclic
    ownership; R is the ownership unit of the sharded step on the long route."""
    return _long_partial_plan(N, T, d, dyadic_order, static_kind, tile_stride, may_refuse=False)


def gram_long_partial_takes(N: int, T: int, d: int, dyadic_order: int = 0, static_kind: int = _lib.STATIC_RBF,
                            tile_stride: int = 1) -> bool:
    """Whether `gram_long_sym_partial` takes N paths [T, d] with these settings: the library's plan query, host only.  False
    exactly where it reports SIGSVGD_E_UNSUPPORTED (past 8192 refined cells on a side, or per-wave state beyond the LDS); any
    other error raises."""
    return _long_partial_plan(N, T, d, dyadic_order, static_kind, tile_stride, may_refuse=True) is not None


def gram_long_sym_partial(X, inv_h: float, tile_offset: int, tile_stride: int, dyadic_order: int = 0,
                          static_kind: int = _lib.STATIC_RBF, grad_out: Optional[torch.Tensor] = None, naive: bool = False,
                          sym: bool = False, out=None, fold: bool = False):
    """This rank's share of the Y-is-X Gram + gradient of the long route on the gathered particles X [N,T,d]
    (`sigsvgd_gram_long_sym_partial`): returns (K_partial [N,N] X.dtype, grad_partial [N,T,d] fp64), zero outside the owned
    pairs.  Summed over tile_offset = 0..tile_stride-1 they equal gram_long_fwd_bwd2(X, X, y_is_x=True): K bit for bit, the
    gradient up to the order of the fp64 sums.  Any T >= 2, dyadic order and built-in static kernel the long route takes.
    The launch owns the row tiles (`gram_long_partial_tiles(...)[0]` rows each) tile_offset + k*tile_stride; with fold=True
    also their mirror images, which gives every rank the same number of pairs (SIGSVGD_FLAG_FOLD_TILES).
    `out=(K_partial, grad_partial)` reuses the caller's buffers (K_partial is re-zeroed, grad_partial overwritten)."""
    dev = _require_gpu(X, grad_out)
    Xc, _ = _prep_long(X, X)
    N, T, d = Xc.shape
    go = _weights(grad_out, (N, N), Xc.dtype)
    Kp, gp = _partial_out(out, Xc, dev)
    flags = _flags(naive=naive, sym=sym, y_is_x=True, fold=fold)
    _launch(dev, "gram_long_sym_partial", (Xc.data_ptr(), N, T, d, _io_dtype(Xc), float(inv_h), int(dyadic_order),
                                           int(static_kind), flags, int(tile_offset), int(tile_stride), _ptr(go),
                                           Kp.data_ptr(), gp.data_ptr()),
            "gram_long_partial_workspace_bytes", (N, T, d, int(dyadic_order), int(static_kind), flags, int(tile_offset),
                                                  int(tile_stride)))
    return Kp, gp


def sym_tile_rows(T: int, d: int) -> int:
    """Rows per tile of the symmetric / partial solve (the ownership unit of the sharded step); 0 for shapes the partial
    solve does not take.  Host-only query of the library."""
    try:
        return int(_lib.load().sigsvgd_gram_sym_tile_rows(int(T), int(d)))
    except RuntimeError:
        # Host-only rule, restated for boxes without the built library (the CPU test doubles of tests/helpers.py and the gloo
        # rehearsal use it to mirror the ownership; every compute entry point still raises without the library):
        # csrc/gram_fast.hip grad_nw (T <= 64: 8 rows, 4 with d > 8), csrc/gram_quad.hip (65 <= T <= 128: 8 rows)
        T, d = int(T), int(d)
        if 3 <= T <= 64 and d <= 16:
            return 8 if d <= 8 else 4
        if 65 <= T <= 128 and d <= 16:
            return 8
        return 0


def owned_tiles(ntile: int, tile_offset: int, tile_stride: int, fold: bool = False):
    """The row tiles `gram_sym_partial(..., tile_offset, tile_stride, fold=)` owns, in the library's order (mirror of
    csrc/sig_common.h TileMap; used by the sharding tests and the CPU test doubles)."""
    first = [t for t in range(tile_offset, ntile, tile_stride) if not fold or t <= (ntile - 1) // 2]
    second = [ntile - 1 - t for t in range(tile_offset, ntile, tile_stride) if 2 * t < ntile - 1] if fold else []
    return first + second


# ---- vector kernels / truncated signature ---------------------------------------
def _prep_vec(t: torch.Tensor, dtype=None) -> torch.Tensor:
    t = t.detach()
    if t.dim() < 2:
        t = torch.atleast_2d(t)
    t = t.flatten(1)
    if dtype is not None and t.dtype != dtype:
        t = t.to(dtype)
    return t.contiguous()


def vec_sqdist(X, Y, XM=None, YM=None) -> torch.Tensor:
    """sq[A,B] = clamp(sum_c (XM - YM)_c (X - Y)_c, 0); XM = YM = None: |x_i - y_j|^2.  X [A,D], Y [B,D]."""
    dev = _require_gpu(X, Y, XM, YM)
    Xc = _prep_vec(X)
    dt = _io_dtype(Xc)
    Yc = _prep_vec(Y, Xc.dtype)
    if Xc.shape[1] != Yc.shape[1]:
        raise ValueError(f"X and Y must share the feature size, got {tuple(Xc.shape)} vs {tuple(Yc.shape)}")
    if (XM is None) != (YM is None):
        raise ValueError("XM and YM must both be given or both be None")
    XMc = YMc = None
    if XM is not None:
        XMc, YMc = _prep_vec(XM, Xc.dtype), _prep_vec(YM, Xc.dtype)
        if XMc.shape != Xc.shape or YMc.shape != Yc.shape:
            raise ValueError("XM / YM must have the shapes of X / Y")
    A, D = Xc.shape
    B = Yc.shape[0]
    if A == 0 or B == 0 or D == 0:
        raise ValueError("empty batch")
    sq = torch.empty((A, B), dtype=Xc.dtype, device=dev)
    _launch(dev, "vec_sqdist", (Xc.data_ptr(), Yc.data_ptr(), _ptr(XMc), _ptr(YMc), A, B, D, dt, sq.data_ptr()))
    return sq


def vec_kernel(sq, XM, YM, kind: int, inv_h2: float, grad_scale: float, grad_out=None, want_K: bool = True,
               want_grad: bool = True):
    """(K[A,B] or None, dK[A,D] or None): K = f(sq), dK = grad_scale * sum_j grad_out_ij w(sq_ij) (XM_i - YM_j)."""
    dev = _require_gpu(sq, XM, YM, grad_out)
    sqc = sq.detach().contiguous()
    dt = _io_dtype(sqc)
    A, B = sqc.shape
    XMc = YMc = None
    D = 1
    if want_grad:
        XMc, YMc = _prep_vec(XM, sqc.dtype), _prep_vec(YM, sqc.dtype)
        D = XMc.shape[1]
        if XMc.shape[0] != A or YMc.shape != (B, D):
            raise ValueError(f"XM {tuple(XMc.shape)} / YM {tuple(YMc.shape)} do not match sq {tuple(sqc.shape)}")
    go = _weights(grad_out, (A, B), sqc.dtype)
    K = torch.empty((A, B), dtype=sqc.dtype, device=dev) if want_K else None
    dK = torch.empty((A, D), dtype=sqc.dtype, device=dev) if want_grad else None
    _launch(dev, "vec_kernel", (sqc.data_ptr(), _ptr(XMc), _ptr(YMc), _ptr(go), A, B, D, dt, int(kind), float(inv_h2),
                                float(grad_scale), _ptr(K), _ptr(dK)))
    return K, dK


def vec_fused_supported(X: torch.Tensor) -> bool:
    """Shapes / dtypes `vec_kernel_fused` takes (include/sigsvgd_hip.h): fp32, up to 512 channels."""
    return X.dtype == torch.float32 and 1 <= X.reshape(X.shape[0], -1).shape[1] <= 512


def vec_kernel_fused(X, Y, kind: int, inv_h2: float, grad_scale: float, XM=None, YM=None, grad_out=None,
                     want_K: bool = True, want_grad: bool = True, reproducible: bool = True):
    """(K[A,B] or None, dK[A,D] or None) for a GIVEN bandwidth in one launch (`sigsvgd_vec_kernel_fused`): the
    distance never goes to HBM and both GEMM-shaped sums run on the fp32 matrix cores.  XM / YM = X M / Y M for the
    scaled kernels (both or neither).  reproducible (default): the column splits of the launch store their partial sums
    in a workspace and a second small launch adds them in a fixed order -- two calls return the same bits; False: one
    launch, the splits meet in fp32 atomics."""
    dev = _require_gpu(X, Y, XM, YM, grad_out)
    Xc, Yc = _prep_vec(X, torch.float32), _prep_vec(Y, torch.float32)
    A, D = Xc.shape
    B = Yc.shape[0]
    if Yc.shape[1] != D:
        raise ValueError(f"X {tuple(Xc.shape)} / Y {tuple(Yc.shape)} channel mismatch")
    if (XM is None) != (YM is None):
        raise ValueError("XM and YM must both be given or both be None")
    XMc = YMc = None
    if XM is not None:
        XMc, YMc = _prep_vec(XM, torch.float32), _prep_vec(YM, torch.float32)
        if XMc.shape != Xc.shape or YMc.shape != Yc.shape:
            raise ValueError(f"XM {tuple(XMc.shape)} / YM {tuple(YMc.shape)} do not match X / Y")
    go = _weights(grad_out, (A, B), torch.float32)
    K = torch.empty((A, B), dtype=torch.float32, device=dev) if want_K else None
    dK = torch.empty((A, D), dtype=torch.float32, device=dev) if want_grad else None
    args = (Xc.data_ptr(), Yc.data_ptr(), _ptr(XMc), _ptr(YMc), _ptr(go), A, B, D, _lib.F32, int(kind), float(inv_h2),
            float(grad_scale), _ptr(K), _ptr(dK))
    if want_grad and reproducible:  # per-split partial sums joined in a fixed order (the header's reproducible route)
        _launch(dev, "vec_kernel_fused", args, "vec_fused_workspace_bytes", (A, B, D))
    else:  # no workspace: the splits meet in atomics (or there is no gradient to split)
        _launch(dev, "vec_kernel_fused", (*args, None, 0))
    return K, dK


def _signature_query(N: int, Ln: int, C: int, depth: int, basepoint: bool, dt: int) -> int:
    """channels of the signature: the entry point itself, asked without data (host only)"""
    n = ctypes.c_longlong(0)
    _lib.check(_lib.load().sigsvgd_signature(None, N, Ln, C, int(depth), int(bool(basepoint)), dt, None, ctypes.byref(n),
                                             None), "signature (channel query)")
    return int(n.value)


def signature_channels(channels: int, depth: int) -> int:
    return _signature_query(1, 1, int(channels), depth, False, _lib.F32)


def _signature_fwd(Xc: torch.Tensor, depth: int, basepoint: bool) -> torch.Tensor:
    dev = Xc.device
    dt = _io_dtype(Xc)
    N, Ln, C = Xc.shape
    out = torch.empty((N, _signature_query(N, Ln, C, depth, basepoint, dt)), dtype=Xc.dtype, device=dev)
    _launch(dev, "signature", (Xc.data_ptr(), N, Ln, C, int(depth), int(bool(basepoint)), dt, out.data_ptr(), None))
    return out


def signature_backward(X, grad_sig, depth: int, basepoint: bool = False) -> torch.Tensor:
    """d sum(grad_sig * signature(X, depth, basepoint)) / dX  -> [N, L, C] (`sigsvgd_signature_backward`)."""
    dev = _require_gpu(X, grad_sig)
    Xc = X.detach().contiguous()
    dt = _io_dtype(Xc)
    N, Ln, C = Xc.shape
    g = grad_sig.detach().to(Xc.dtype).contiguous()
    if g.dim() != 2 or g.shape[0] != N or g.shape[1] != signature_channels(C, depth):
        raise ValueError(f"grad_sig must be [{N}, {signature_channels(C, depth)}], got {tuple(g.shape)}")
    gX = torch.empty_like(Xc)
    _launch(dev, "signature_backward", (Xc.data_ptr(), g.data_ptr(), N, Ln, C, int(depth), int(bool(basepoint)), dt,
                                        gX.data_ptr()))
    return gX


class _Signature(torch.autograd.Function):
    """signature(X) as an autograd node: HIP forward, HIP adjoint (the path is the only differentiable input)."""

    @staticmethod
    def forward(ctx, X, depth, basepoint):
        Xc = X.detach().contiguous()
        ctx.save_for_backward(Xc)
        ctx.depth, ctx.basepoint = int(depth), bool(basepoint)
        return _signature_fwd(Xc, depth, basepoint)

    @staticmethod
    def backward(ctx, grad_sig):
        (Xc,) = ctx.saved_tensors
        return signature_backward(Xc, grad_sig, ctx.depth, ctx.basepoint), None, None


def signature(X, depth: int, basepoint: bool = False) -> torch.Tensor:
    """Truncated signature of paths X [N, L, C] -> [N, C + ... + C^depth] (signatory's layout).  Differentiable with
    respect to X (reference: `signatory.signature` inside PathSigKernel, src/kernels/_traj_kernels.py:124-125, reached by
    autograd from src/inference/score.py:50-55)."""
    _require_gpu(X)
    if X.dim() != 3:
        raise ValueError(f"paths must be [batch, length, channels]; got {tuple(X.shape)}")
    if X.shape[0] == 0:
        raise ValueError("empty batch")
    _io_dtype(X)
    if X.requires_grad and torch.is_grad_enabled():
        return _Signature.apply(X, int(depth), bool(basepoint))
    return _signature_fwd(X.detach().contiguous(), depth, basepoint)


def obstacle_cost(x, start, target, basis, log_weights, mean, std, w_obstacle: float = 1.0, w_length: float = 1.0,
                  want_traj: bool = True, want_grad: bool = True):
    """Planning cost of the reference's obstacle-field script on the device with its analytic gradient
    (`sigsvgd_obstacle_cost`; examples/script_planning_obstacle_field.py:113-126).

    x [N, knots, d] interior knots, start/target [d], basis [samples, knots + 2], mixture log_weights [M]
    (normalised), mean/std [M, d].  Returns (cost [N], traj [N, samples, d] or None, d cost / d x or None)."""
    dev = _require_gpu(x, basis, mean, std, log_weights, start, target)
    if x.dim() != 3:
        raise ValueError(f"knots must be [batch, knots, channels]; got {tuple(x.shape)}")
    N, Kx, d = x.shape
    if N == 0:
        raise ValueError("empty batch")
    f = lambda t: t.detach().to(torch.float32).contiguous()
    xc, bc, mc, sc, lw, st, tg = f(x), f(basis), f(mean), f(std), f(log_weights), f(start).reshape(-1), f(target).reshape(-1)
    if bc.dim() != 2 or bc.shape[1] != Kx + 2:
        raise ValueError(f"basis must be [samples, {Kx + 2}]; got {tuple(bc.shape)}")
    if mc.shape != sc.shape or mc.dim() != 2 or mc.shape[1] != d or lw.numel() != mc.shape[0]:
        raise ValueError(f"mixture mean/std must be [components, {d}] with one log-weight each; got {tuple(mc.shape)}, "
                         f"{tuple(sc.shape)}, {tuple(lw.shape)}")
    if st.numel() != d or tg.numel() != d:
        raise ValueError(f"start and target poses must have {d} channels")
    Tt = bc.shape[0]
    cost = torch.empty(N, dtype=torch.float32, device=dev)
    traj = torch.empty((N, Tt, d), dtype=torch.float32, device=dev) if want_traj else None
    grad = torch.empty((N, Kx, d), dtype=torch.float32, device=dev) if want_grad else None
    _launch(dev, "obstacle_cost", (xc.data_ptr(), N, Kx, d, st.data_ptr(), tg.data_ptr(), bc.data_ptr(), Tt, lw.data_ptr(),
                                   mc.data_ptr(), sc.data_ptr(), mc.shape[0], float(w_obstacle), float(w_length),
                                   cost.data_ptr(), _ptr(traj), _ptr(grad)))
    return cost, traj, grad


# ---- signature PDE on a caller's static-kernel grid (user static kernels) -------------------------
def _prep_grid(G: torch.Tensor) -> torch.Tensor:
    if G.dim() != 3:
        raise ValueError(f"static-kernel grids must be [npairs, M, N]; got {tuple(G.shape)}")
    if G.shape[0] == 0:
        raise ValueError("empty batch")
    if G.shape[1] < 2 or G.shape[2] < 2:
        raise ValueError(f"static-kernel grids need at least 2 x 2 points; got {tuple(G.shape)}")
    _io_dtype(G)
    return G.detach().contiguous()


def pde_fwd(G, dyadic_order: int = 0, naive: bool = False) -> torch.Tensor:
    """K[npairs] = signature kernel of each pair from its static-kernel grid G [npairs, M, N] (`sigsvgd_pde_fwd`): fp64
    increments and sweeps, K in G's dtype."""
    dev = _require_gpu(G)
    Gc = _prep_grid(G)
    npairs, M, N = Gc.shape
    flags = _flags(naive=naive)
    K = torch.empty(npairs, dtype=Gc.dtype, device=dev)
    _launch(dev, "pde_fwd", (Gc.data_ptr(), npairs, M, N, _io_dtype(Gc), int(dyadic_order), flags, K.data_ptr()),
            "pde_workspace_bytes", (npairs, M, N, int(dyadic_order), 0, flags))
    return K


def pde_fwd_bwd(G, dyadic_order: int = 0, grad_out: Optional[torch.Tensor] = None,
                naive: bool = False, exact_adjoint: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """(K[npairs], dG[npairs, M, N]) with dG = d sum(grad_out * K) / dG (`sigsvgd_pde_fwd_bwd`; grad_out None = ones), in
    the reference's convention GG = K_fwd * K_rev (the exact adjoint for the naive stencil; what the built-in kernels
    return), or with exact_adjoint (SIGSVGD_FLAG_EXACT_ADJOINT) the exact derivative of the discrete
    K for the default stencil too; K has the same bits either way.  Bit-reproducible."""
    dev = _require_gpu(G, grad_out)
    Gc = _prep_grid(G)
    npairs, M, N = Gc.shape
    go = None
    if grad_out is not None:
        if grad_out.numel() != npairs:
            raise ValueError(f"grad_out must have {npairs} entries, got {tuple(grad_out.shape)}")
        go = grad_out.detach().reshape(npairs).to(Gc.dtype).contiguous()
    flags = _flags(naive=naive, exact_adjoint=exact_adjoint)
    K = torch.empty(npairs, dtype=Gc.dtype, device=dev)
    dG = torch.empty_like(Gc)
    _launch(dev, "pde_fwd_bwd", (Gc.data_ptr(), npairs, M, N, _io_dtype(Gc), int(dyadic_order), flags, _ptr(go),
                                 K.data_ptr(), dG.data_ptr()),
            "pde_workspace_bytes", (npairs, M, N, int(dyadic_order), 1, flags))
    return K, dG


class PDESolve(torch.autograd.Function):
    """K[...] = signature kernel of every static-kernel grid G[..., M, N] (any leading shape).  Backward: dG from one
    `pde_fwd_bwd` launch with the incoming weights, so gradients reach whatever produced G -- the paths through a user's
    `Gram_matrix`, and that static kernel's own parameters.  exact_adjoint: as `pde_fwd_bwd`'s."""

    @staticmethod
    def forward(ctx, G, dyadic_order, naive, exact_adjoint=False):
        lead, (M, N) = tuple(G.shape[:-2]), tuple(G.shape[-2:])
        Gf = G.detach().reshape(-1, M, N)
        ctx.cfg = (lead, int(dyadic_order), bool(naive))
        ctx.exact_kw = {"exact_adjoint": True} if exact_adjoint else {}
        ctx.save_for_backward(Gf)
        return pde_fwd(Gf, dyadic_order, naive).reshape(lead)

    @staticmethod
    def backward(ctx, grad_output):
        (Gf,) = ctx.saved_tensors
        lead, dyadic_order, naive = ctx.cfg
        _, dG = pde_fwd_bwd(Gf, dyadic_order, grad_output.reshape(-1), naive, **ctx.exact_kw)
        return dG.reshape(lead + tuple(Gf.shape[-2:])), None, None, None
