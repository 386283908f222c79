"""Test doubles: oracle-backed CPU stand-ins for `sigsvgd_amd.ops`, used ONLY by the `-m "not gpu"`
host-logic tests (the product has no CPU path; these live under tests/ on purpose)."""
import os

import numpy as np
import torch

from oracle import sigkernel_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_fixtures.npz")


def golden():
    return np.load(GOLDEN, allow_pickle=False)


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def gram_fwd(X, Y, inv_h, dyadic_order=0, static_kind=0, naive=False, force_generic=False, y_is_x=False):
    K = O.gram(_np(X), _np(Y), static_kind, 1.0 / inv_h, dyadic_order, naive)
    return torch.as_tensor(K, dtype=X.dtype)


def gram_fwd_bwd(X, Y, inv_h, dyadic_order=0, static_kind=0, grad_out=None, naive=False, sym=False,
                 y_is_x=False, force_generic=False):
    go = None if grad_out is None else _np(grad_out)
    K, g = O.gram_backward(_np(X), _np(Y), go, static_kind, 1.0 / inv_h, dyadic_order, naive, sym)
    return torch.as_tensor(K, dtype=X.dtype), torch.as_tensor(g, dtype=X.dtype)


def svgd_phi(K, score, grad_k, mask=None, X=None, lr=None, adagrad_state=None):
    N = K.shape[0]
    v = -((K.float() @ score.float().reshape(N, -1) - grad_k.float().reshape(N, -1)) / N)
    if mask is not None:
        v = v * torch.broadcast_to(torch.as_tensor(mask, dtype=torch.float32), score.shape).reshape(N, -1)
    if adagrad_state is not None:
        adagrad_state += (v * v).reshape(adagrad_state.shape)
        v = v / torch.sqrt(adagrad_state.reshape(N, -1) + 1e-12)
    v = v.reshape(score.shape)
    if X is not None:
        return v, X.float() - lr * v
    return v


def gram_sym_partial(X, inv_h, tile_offset, tile_stride, static_kind=0, grad_out=None, sym=False, out=None, fold=False):
    """Same ownership rule as the HIP kernels, taken from the library itself (host-only queries): unordered pairs
    {i <= j} whose row tile of i -- `ops.sym_tile_rows(T, d)` rows -- is one of `ops.owned_tiles(...)`."""
    from sigsvgd_amd import ops

    Xn = _np(X)
    N, T, d = Xn.shape
    nw = ops.sym_tile_rows(T, d)
    owned = set(ops.owned_tiles((N + nw - 1) // nw, tile_offset, tile_stride, fold))
    Kp = np.zeros((N, N))
    gp = np.zeros((N, T, d))
    for i in range(N):
        if (i // nw) not in owned:
            continue
        for j in range(i, N):
            Kij, gi = O.gram_backward(Xn[i:i + 1], Xn[j:j + 1], None, static_kind, 1.0 / inv_h, 0)
            Kp[i, j] = Kp[j, i] = Kij[0, 0]
            gp[i] += gi[0]
            if j != i:
                _, gj = O.gram_backward(Xn[j:j + 1], Xn[i:i + 1], None, static_kind, 1.0 / inv_h, 0)
                gp[j] += gj[0]
    Kt, gt = torch.as_tensor(Kp, dtype=X.dtype), torch.as_tensor(gp, dtype=torch.float64)
    if out is not None:
        out[0].copy_(Kt)
        out[1].copy_(gt)
        return out
    return Kt, gt


def patch_ops(monkeypatch):
    """Replace the HIP-backed ops by the oracle-backed doubles (CPU host-logic tests only)."""
    from sigsvgd_amd import ops

    for name, fn in [("gram_fwd", gram_fwd), ("gram_fwd_bwd", gram_fwd_bwd), ("svgd_phi", svgd_phi),
                     ("gram_sym_partial", gram_sym_partial)]:
        monkeypatch.setattr(ops, name, fn)


def ring_plan(M, N, n, want_grad, row_doubles, cus):
    """The geometry of csrc/ring_sweep.h (`ring_make_plan`) for M x N coarse grids at order n on `cus` compute units, as a
    dict (P, Q, nrow, W, lds, per_wave, resident), or None where the library refuses the launch (E_UNSUPPORTED).
    `row_doubles`: the caller's LDS per point of a band's nrow + 1 coarse rows (0 for sig_pde, d for gram_long)."""
    r = 1 << n
    P, Q = r * (M - 1), r * (N - 1)
    if P > 8192 or Q > 8192:
        return None
    nrow = 64 >> n if n <= 6 else 1
    W = 1
    while W < N - 1:
        W <<= 1
    Wcap = 1
    while Wcap * 2 * nrow <= 8192:
        Wcap <<= 1
    W = min(W, Wcap)
    lds = (nrow * W + Q + 2 + 64 + (nrow + 1) * row_doubles) * 8
    if lds > 160 * 1024:
        return None
    per_wave = (2 * -(-P // 64) * (Q + 63) * 64 + 64) * 4 if want_grad else 0
    return dict(P=P, Q=Q, nrow=nrow, W=W, lds=lds, per_wave=per_wave, resident=cus * min(160 * 1024 // lds, 8))


def long_plan(A, B, M, N, d, n, want_grad=True, cus=256):
    """The launch plan of csrc/gram_long.hip (`long_make_plan`) for X [A, M, d] x Y [B, N, d] on `cus` compute units, as a
    dict (nrow, W, JC, nchunks, items, grid, lds, bytes), or None where the library refuses the launch (E_UNSUPPORTED).
    `bytes` is what sigsvgd_gram_long_workspace_bytes reports; tests/test_long_cabi.py pins the two together."""
    pl = ring_plan(M, N, n, want_grad, d, cus)
    if pl is None:
        return None
    JC = 32
    while JC > 1 and A * -(-B // JC) < pl["resident"]:
        JC >>= 1
    nchunks = -(-B // JC)
    grid = min(pl["resident"], A * nchunks)
    if want_grad and pl["per_wave"] * grid > (1 << 30):
        grid = max(1, (1 << 30) // pl["per_wave"])
    wsk_bytes = (pl["per_wave"] * grid + 255) & ~255
    partial_bytes = A * nchunks * M * d * 8 if want_grad else 0
    total = wsk_bytes + partial_bytes + 256 if wsk_bytes + partial_bytes else 0
    return dict(pl, JC=JC, nchunks=nchunks, items=A * nchunks, grid=grid, bytes=total)


def pair_plan(A, M, N, d, n, want_grad=True, cus=256):
    """The paired launch plan of csrc/gram_long.hip (`pair_make_plan`) for X [A, M, d] and Y [A, N, d] on `cus` compute
    units, as a dict (P, Q, nrow, W, resident, grid, lds, bytes), or None where the library refuses the launch (E_UNSUPPORTED).
    One pair per wavefront: grid = min(resident waves, A), lowered to keep the per-wave scratch within 1 GiB; no slabs."""
    pl = long_plan(A, 1, M, N, d, n, want_grad, cus)
    if pl is None:
        return None
    wsk_bytes = (pl["per_wave"] * pl["grid"] + 255) & ~255
    return dict(pl, bytes=wsk_bytes + 256 if wsk_bytes else 0)


def pde_plan(npairs, M, N, n, want_grad=True, cus=256):
    """The launch plan of csrc/sig_pde.hip (`pde_make_plan`) for npairs grids [M, N] on `cus` compute units, as a dict
    (nrow, W, grid, lds, bytes), or None where the library refuses the launch.  `bytes` is what sigsvgd_pde_workspace_bytes
    reports; tests/test_pde_cabi.py pins the two together."""
    pl = ring_plan(M, N, n, want_grad, 0, cus)
    if pl is None:
        return None
    per_wave = pl["per_wave"]
    slots = min(cus * 8, npairs)
    ws = per_wave * slots
    if ws > (1 << 30):
        slots = max(1, (1 << 30) // per_wave)
        ws = max(per_wave, 1 << 30)
    return dict(pl, grid=min(pl["resident"], slots), bytes=ws + 256 if ws else 0)


def device_cus():
    """The compute units the library plans for: the device's count, or its fallback of 256 without a device."""
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
