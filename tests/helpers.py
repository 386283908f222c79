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


# ---- launch geometry of the fp32-sweep Gram kernels (gram_fast / gram_quad / gram_dyad / gram_band) ----------------------
def _band_lds(T, P, dpad, serial_slots):
    """(pair0, per_pair, total) bytes of csrc/gram_band.hip's LDS layout (`bandp_lds`); serial_slots 0 = band-parallel"""
    def up16(b):
        return (b + 15) & ~15

    Tm, rows, nb = T - 1, T * dpad, (P + 63) >> 6
    hrows = 1 if serial_slots else max(nb - 1, 1)
    ndump = 1 if serial_slots else nb
    hn = 2 * 64 + 64 * ((P + 62) // 64) + 80
    pair0 = up16(T * (dpad + 1) * 8) + up16(dpad * 8) + up16(rows * 4)
    w = up16(Tm * Tm * 8) + 64
    dtab = (Tm + 1) * (Tm + 2 * (80 // (P // Tm) + 2))
    w += up16(max(dtab, rows) * 4)
    hK = w
    w += 2 * up16(hrows * hn * 4)
    w = max(w, hK + up16((T * T + rows) * 4))
    w += up16(rows * 4) + ndump * 96 * 4
    return pair0, w, pair0 + (serial_slots or 1) * w


def _band_serial_slots(T, d, n):
    pair0, per_pair, _ = _band_lds(T, (T - 1) << n, 8 if d <= 8 else 16, 1)
    return max(1, min(8, (158 * 1024 - pair0) // per_pair))


def _band_wg_per_cu(T, d, n, serial):
    """`band_wg_per_cu` restated in full (LDS bound and wavefront bound), not its upper bound 16 / wavefronts"""
    P = (T - 1) << n
    slots = _band_serial_slots(T, d, n) if serial else 0
    total = _band_lds(T, P, 8 if d <= 8 else 16, slots)[2]
    return max(1, min(160 * 1024 // (total + 1024), 16 // (slots if serial else (P + 63) >> 6)))


def gram_geometry(A, B, T, d, n, want_grad, sym, cus=256, band_mode=None):
    """The work split of a Gram launch (RBF, second-order solver) of X [A, T, d] x Y [B, T, d] at dyadic order n on `cus`
    compute units, as a dict (family, rows_per_tile, resident, items, grid); None where the launch leaves the four fp32-sweep
    families for the coverage kernel.  `sym`: the Y_IS_X orientation (A == B, each unordered pair once).  Restates
    `gram_route` (csrc/capi.hip), `dispatch_variant` / `launch_variant` / `grad_nw` / `grad_wg_per_cu` (gram_fast.hip),
    `quad_plan`, `dyad_plan` and `band_geometry`; a launch is `items` (row tile, column) pairs over
    grid = min(items, resident) workgroups, workgroup w taking the items [items*w/grid, items*(w+1)/grid).
    `band_mode`: SIGSVGD_BAND_MODE ("serial" / "parallel"; None: the environment's).
    tests/test_gram_geometry.py pins it to the library's workspace queries."""
    if band_mode is None:
        band_mode = os.environ.get("SIGSVGD_BAND_MODE", "")
    P = (T - 1) << n
    if want_grad and d == 1 and n == 0 and 3 <= T <= 128:
        return None  # one-channel gradients: the coverage kernel
    small = 3 <= T <= 33 and d <= 16
    if n == 0 and 3 <= T <= 64 and d <= 16:
        family = "fast"
        if want_grad:
            rows, per_cu = (8 if d <= 8 else 4), (3 if d <= 8 and T <= 32 else 1)
        elif d <= 8:  # forward only: 4-wave workgroups, two rows per wavefront on the 32-slot ring
            rows, per_cu = (8 if T <= 32 else 4), 3
        else:
            rows, per_cu = 4, 2
    elif n == 0 and 65 <= T <= 128 and d <= 16:
        family, rows, per_cu = "quad", 8, 1
    else:
        dyad = small and 1 <= n <= 6 and 64 <= P <= 128
        band = small and 2 <= n <= 7 and 64 <= P <= 256
        pairs = A * (A + 1) // 2 if sym else A * B
        nb = (P + 63) >> 6
        if band_mode[:1] == "s":
            parallel = False
        elif band_mode[:1] == "p" or nb <= 2:
            parallel = True
        else:
            parallel = 2 * pairs <= (3 if nb >= 4 else 10) * cus * _band_wg_per_cu(T, d, n, False)
        if dyad and not (band and (P > 64 or d == 1) and parallel):
            family, rows, per_cu = "dyad", (4 if pairs <= 4 * cus else 8), 1
        elif band:
            family = "band parallel" if parallel else "band serial"
            rows = 1 if parallel else _band_serial_slots(T, d, n)
            per_cu = _band_wg_per_cu(T, d, n, not parallel)
        else:
            return None
    ntile = -(-A // rows)
    items = sum(B - t * rows for t in range(ntile)) if sym else ntile * B
    resident = cus * per_cu
    return dict(family=family, rows_per_tile=rows, resident=resident, items=items, grid=min(items, resident))


def gram_item_ranges(A, B, geom, sym, tiles=None):
    """(bounds, starts) of a launch with geometry `geom` (gram_geometry): workgroup w works on the items
    [bounds[w], bounds[w + 1]); the k-th tile is the items [starts[k], starts[k + 1]) -- ordered launches all B columns,
    symmetric ones the columns from the tile's first row on.  `tiles`: the row tiles a partial solve owns, in its order
    (`ops.owned_tiles`; geom then carries that launch's items and grid); None: all of them."""
    rows, items, grid = geom["rows_per_tile"], geom["items"], geom["grid"]
    tiles = range(-(-A // rows)) if tiles is None else tiles
    starts = np.concatenate([[0], np.cumsum([B - t * rows if sym else B for t in tiles])]).astype(np.int64)
    bounds = items * np.arange(grid + 1, dtype=np.int64) // grid
    assert starts[-1] == items
    return bounds, starts


def gram_multi_item_regime(A, B, geom, sym, tiles=None):
    """The four conditions under which a launch exercises the kernels' loop over items: at least 2 * grid + 1 items, a
    workgroup range that starts strictly inside a tile, one that crosses from a tile into the next, and a tile met by two or
    more workgroups.  -> dict of booleans (multi, inside, crosses, shared)."""
    bounds, starts = gram_item_ranges(A, B, geom, sym, tiles)
    lo, hi = bounds[:-1], bounds[1:]
    inner = starts[1:-1]  # the tile boundaries inside the launch
    first_wg = np.searchsorted(hi, starts[:-1], side="right")  # workgroup holding a tile's first item
    last_wg = np.searchsorted(hi, starts[1:] - 1, side="right")  # ... and its last
    return dict(multi=bool(geom["items"] >= 2 * geom["grid"] + 1), inside=bool((~np.isin(lo, starts)).any()),
                crosses=bool(((lo[:, None] < inner[None, :]) & (inner[None, :] < hi[:, None])).any()),
                shared=bool((last_wg > first_wg).any()))


def gram_ordered_grad_bytes(A, B, T, d, n, cus=256, band_mode=None):
    """What sigsvgd_gram_workspace_bytes reports for an ordered (A != B) gradient query on the four fp32-sweep families:
    [A][B] flag bytes (register-resident kernel: d <= 4 only), fp64 row segments of (tiles + grid) * rows_per_tile paths,
    the family's scratch, and 256 bytes of alignment slack."""
    def r256(b):
        return (b + 255) & ~255

    assert A != B
    g = gram_geometry(A, B, T, d, n, True, False, cus, band_mode)
    rows = g["rows_per_tile"]
    total = r256((-(-A // rows) + g["grid"]) * rows * T * d * 8) + 256
    if g["family"] != "fast" or d <= 4:
        total += r256(A * B)
    if g["family"] == "quad":  # increment scratch of 3 quadrants per row and workgroup; row accumulators for d = 15, 16
        total += cus * 8 * 6 * 64 * 64 * 4 + (cus * 8 * 128 * 16 * 4 if d > 14 else 0)
    if g["family"].startswith("band"):  # forward solution of the pairs in flight: whole phases of 16 steps per band
        P = (T - 1) << n
        per_pair = ((P + 63) >> 6) * (-(-(P + 63) // 16) * 16) * 64 + 32 * 64
        total += r256(g["grid"] * rows * per_pair * 4)
    return total


def signed_weights(A, B, seed):
    """grad_out with every entry of the same order and random sign: w = s u, s = +-1, u uniform in [0.5, 1.5] -- no pair
    is hidden behind a weight near zero"""
    rng = np.random.default_rng(seed)
    return rng.choice([-1.0, 1.0], size=(A, B)) * rng.uniform(0.5, 1.5, size=(A, B))
