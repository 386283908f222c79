"""Python restatements of the library's launch plans, and the case tables that are read off them.  Each function names the
C++ function it mirrors; the host-only C-ABI tests pin every one of them to the library's own workspace and plan queries
(test_pde_cabi, test_long_cabi, test_long2_cabi, test_long_partial_cabi, test_pair_cabi, test_gram_geometry,
test_generic_plan_cabi), so the GPU tests can assert from them which branch of a plan a shape reaches."""
import os
from collections import namedtuple
from functools import lru_cache

import numpy as np
import torch

from sigsvgd_amd import ops


def device_cus():
    """The compute units the library plans for: the device's count, or its fallback of 256 without a device."""
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256


def set_band_mode(monkeypatch, mode):
    """SIGSVGD_BAND_MODE for the test ("serial" / "parallel"; None: unset, the launcher's own rule)"""
    if mode is None:
        monkeypatch.delenv("SIGSVGD_BAND_MODE", raising=False)
    else:
        monkeypatch.setenv("SIGSVGD_BAND_MODE", mode)


def tiles(n, c):
    return -(-n // c)


# ---- the long-path sweeps (ring_sweep.h) and the plans built on them -------------------------------------------------------
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


def long2_plan(A, B, M, N, d, n, want_x=True, want_y=True, yx=False, cus=256):
    """The launch plan of csrc/gram_long.hip's two-sided mode (`long2_make_plan`) on top of ring_plan, as a dict (IC,
    JC, nti, ntj, items, grid, slab_bytes, bytes), or None where the library refuses the launch (E_UNSUPPORTED).  Tiles of
    IC rows x JC columns, the largest powers of two <= 32 that still give every resident wave an item (the wider side is
    halved first); yx: square tiles of the upper triangle, and a row keeps nti + 1 slabs."""
    want_grad = want_x or want_y
    pl = ring_plan(M, N, n, want_grad, d, cus)
    if pl is None:
        return None
    IC = JC = 32
    if yx:
        tri = lambda c: tiles(A, c) * (tiles(A, c) + 1) // 2
        while IC > 1 and tri(IC) < pl["resident"]:
            IC >>= 1
        JC, items = IC, tri(IC)
    else:
        while (IC > 1 or JC > 1) and tiles(A, IC) * tiles(B, JC) < pl["resident"]:
            if JC >= IC:
                JC >>= 1
            else:
                IC >>= 1
        items = tiles(A, IC) * tiles(B, JC)
    nti, ntj = tiles(A, IC), tiles(B, JC)
    grid = min(pl["resident"], items)
    if want_grad and pl["per_wave"] * grid > (1 << 30):
        grid = max(1, (1 << 30) // pl["per_wave"])
    wsk_bytes = (pl["per_wave"] * grid + 255) & ~255
    if yx:
        slab_bytes = A * (nti + 1) * M * d * 8 if want_grad else 0
    else:
        slab_bytes = (A * ntj * M * d * 8 if want_x else 0) + (B * nti * N * d * 8 if want_y else 0)
    total = wsk_bytes + slab_bytes
    return dict(pl, IC=IC, JC=JC, nti=nti, ntj=ntj, items=items, grid=grid, slab_bytes=slab_bytes,
                bytes=total + 256 if total else 0)


# ---- the mirror of csrc/gram_long.hip's partial plan -------------------------------------------------------------------
def part_items(N, R, JC, owned):
    """The items (kq, c) of a launch that owns the row tiles `owned` (R rows each), in the order the kernel takes them
    (`part_decode`): the chunks strictly between a tile's first and last, then every tile's first chunk, then the last."""
    nc = [tiles(N - t * R, JC) for t in owned]
    out = [(k, c) for k in range(len(owned)) for c in range(1, nc[k] - 1)]
    out += [(k, 0) for k in range(len(owned))]
    out += [(k, nc[k] - 1) for k in range(len(owned)) if nc[k] >= 2]
    return out


def item_pairs(N, R, JC, t, c):
    """The pairs of item (row tile t, chunk c) in the order the kernel walks them: row by row, i <= j only."""
    i0, i1 = t * R, min(N, (t + 1) * R)
    j0 = i0 + c * JC
    j1 = min(N, j0 + JC)
    return [(i, j) for i in range(i0, i1) for j in range(max(j0, i), j1)]


def item_size(N, R, JC, t, c):
    i0, i1 = t * R, min(N, (t + 1) * R)
    j0 = i0 + c * JC
    j1 = min(N, j0 + JC)
    whole = max(0, min(i1, j0 + 1) - i0)  # rows at or above the chunk's first column: j1 - j0 pairs each
    lo, hi = max(i0, j0 + 1), min(i1, j1) - 1  # rows cut by the diagonal: j1 - i pairs
    cut = (hi - lo + 1) * j1 - (lo + hi) * (hi - lo + 1) // 2 if hi >= lo else 0
    return whole * (j1 - j0) + cut


def part_share(N, R, JC, off, stride, fold, res):
    """One rank's share: dict(pairs, makespan, slabs, items, owned); slabs in units of T * d doubles (a row-side slab per
    (row of an owned tile, chunk), a column-side slab per (owned tile, row from the tile's first on)); makespan = the most
    pairs one wavefront walks when item k goes to wave k % grid, grid = min(resident waves, items)."""
    owned = ops.owned_tiles(tiles(N, R), off, stride, fold)
    sizes = [item_size(N, R, JC, owned[k], c) for (k, c) in part_items(N, R, JC, owned)]
    slabs = sum((min(N, (t + 1) * R) - t * R) * tiles(N - t * R, JC) + (N - t * R) for t in owned)
    grid = max(1, min(res, len(sizes)))
    load = [0] * grid
    for k, p in enumerate(sizes):
        load[k % grid] += p
    return dict(pairs=sum(sizes), makespan=max(load), slabs=slabs, items=len(sizes), owned=owned)


@lru_cache(maxsize=None)
def part_pick(N, stride, res):
    """(R, JC) of `part_pick`: the largest R * JC (ties: the larger R) whose every rank, folded, meets the schedule
    (eff >= 0.9), memory and balance (fullest <= 1.05 x mean) conditions; else, memory holding, best balance then schedule."""
    cands = sorted(((R, JC) for R in (32, 16, 8, 4, 2, 1) for JC in range(64, 0, -1)), key=lambda x: -x[0] * x[1])
    total = N * (N + 1) // 2
    best, best_key = (1, 1), None
    for (R, JC) in cands:
        if R > 1 and tiles(N, R) < 2 * stride:
            continue
        shares = [part_share(N, R, JC, off, stride, True, res) for off in range(stride)]
        if not all(s["slabs"] <= (N * N // 4 if s["pairs"] > 16 * res else 2 * s["pairs"] + N) for s in shares):
            continue
        eff = min([1.0] + [-(-s["pairs"] // res) / s["makespan"] for s in shares if s["pairs"]])
        bal = max(s["pairs"] for s in shares) * stride <= 1.05 * total
        if eff >= 0.9 and bal:
            return R, JC
        if best_key is None or (bal, eff) > best_key:
            best, best_key = (R, JC), (bal, eff)
    return best


def part_plan(N, T, d, n, off, stride, fold, cus=256):
    """The plan of rank `off` of `stride` (`part_make_plan`) as a dict (R, JC, items, grid, pairs, makespan, eff, slabs,
    bytes), or None where the library refuses the launch."""
    pl = ring_plan(T, T, n, True, d, cus)
    if pl is None:
        return None
    res = pl["resident"]
    R, JC = part_pick(N, stride, res)
    sh = part_share(N, R, JC, off, stride, fold, res)
    grid = min(res, sh["items"])
    if pl["per_wave"] * grid > (1 << 30):
        grid = max(1, (1 << 30) // pl["per_wave"])
    total = ((pl["per_wave"] * grid + 255) & ~255) + sh["slabs"] * T * d * 8
    eff = -(-sh["pairs"] // res) / sh["makespan"] if sh["pairs"] else 1.0
    return dict(pl, R=R, JC=JC, grid=grid, eff=eff, bytes=total + 256 if total else 0, **sh)


# ---- the branches of long_plan / long2_plan that tests/test_gpu_long.py and test_gpu_long2.py run ---------------------------
def oracle_at_own_lengths(X, Y, h, n, naive, kind, go, nthreads=0):
    """The C oracle for X [A, TX, d] x Y [B, TY, d]: the shorter batch padded with its last point (exact,
    `ops.pad_to_length`), the gradient of a padded X folded back onto its points (`ops.fold_padded_grad`)."""
    from oracle import c_oracle

    T = max(X.shape[1], Y.shape[1])
    pad = lambda P: ops.pad_to_length(torch.as_tensor(P), T).numpy()
    Kr, gr = c_oracle.gram_fwd_bwd(pad(X), pad(Y), h=h, n=n, naive=naive, kind=kind, grad_out=go, nthreads=nthreads)
    return Kr, ops.fold_padded_grad(torch.as_tensor(gr), X.shape[1]).numpy()


def branch_regime(tag, pl, M, N):
    """the branch a case is there for, read off the launch plan"""
    return {"full": N - 1 == pl["W"],                       # the ring holds every column exactly: no wrap
            "wrap": N - 1 == pl["W"] + 1,                   # one column more than the ring: wraps once
            "nrow1": pl["nrow"] == 1 and pl["P"] > 64,      # a band of 64 rows is part of one coarse row
            "L1": pl["P"] % 64 == 1 and pl["P"] > 64,       # the last band has one row
            "Q1": pl["Q"] == 1, "P1": pl["P"] == 1,         # a single coarse column / row
            "short_x": M < N, "long_x": M > N,
            "channels": True}[tag]                          # (d = 16 in registers, 17 and 33 from global memory)


# (A, B, TX, TY, d, n, kind, naive, regime); nthreads of the oracle where its tables are large
BRANCH_CASES = [
    # ring: exactly full and wrapping once, at orders 0, 1, 2 (Wcap = 128, 256, 512 columns)
    *[(2, 2, T, T, 2, n, kind, naive, reg) for (T, n, reg) in [(129, 0, "full"), (130, 0, "wrap"), (257, 1, "full"),
                                                              (258, 1, "wrap"), (513, 2, "full"), (514, 2, "wrap")]
      for kind in (0, 1) for naive in (False, True)],
    # orders 7 to 10 (nrow = 1), square and not.  (The default stencil at P = Q = 8192 runs on the 8192 x 2048 grid: on
    #  8192 x 8192 cells the oracle's own sweep, which forms 1 + g/2 + g^2/12 with g ~ D / 2^20, is 0.7 .. 1.5e-9 from a
    #  long-double sweep of the same increments, the kernel's cancellation-free form within 5e-10 of it; on 8192 x 2048
    #  the oracle is within 5e-10.)
    *[(1, 2, 9, 9, 2, n, kind, naive, "nrow1") for n in (7, 8) for kind in (0, 1) for naive in (False, True)],
    *[(1, 2, 9, 9, 2, 10, kind, True, "nrow1") for kind in (0, 1)],
    (2, 2, 5, 9, 2, 8, 0, False, "nrow1"),
    (1, 2, 9, 3, 3, 10, 0, False, "nrow1"),
    (1, 2, 9, 3, 3, 10, 1, True, "nrow1"),
    # a last band of one row; a single coarse column or row against a long path
    (2, 2, 66, 66, 2, 0, 0, False, "L1"),
    (2, 2, 258, 258, 3, 0, 0, True, "L1"),
    (2, 3, 66, 66, 2, 0, 1, False, "L1"),
    (2, 2, 300, 2, 2, 0, 0, False, "Q1"),
    (2, 2, 2, 300, 2, 0, 0, False, "P1"),
    (2, 2, 2, 300, 2, 0, 1, True, "P1"),
    # X shorter than Y, and unequal lengths at refined orders
    (3, 2, 150, 400, 2, 0, 0, False, "short_x"),
    (2, 3, 60, 100, 3, 2, 0, False, "short_x"),
    (2, 2, 40, 70, 2, 1, 1, True, "short_x"),
    (2, 2, 200, 90, 2, 1, 1, False, "long_x"),
    # channels past the 16 the fill keeps in registers (the gradient's 16-channel passes: 1, 2, 3) and at the LDS limit
    *[(2, 2, 300, 300, d, 0, kind, False, "channels") for d in (16, 17, 33) for kind in (0, 1)],
    (1, 2, 300, 300, 183, 0, 0, False, "channels"),
]


def branch_id(c):
    A, B, TX, TY, d, n, kind, naive, reg = c
    return f"{reg}-{A}x{B}-T{TX}x{TY}-d{d}-n{n}-{'lin' if kind else 'rbf'}{'-naive' if naive else ''}"


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
    `gram_route` (csrc/capi.hip), `dispatch_variant` / `launch_variant` (gram_fast_kernel.h), `grad_nw` / `grad_wg_per_cu` (gram_fast.hip),
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


# ---- the coverage kernel (gram_generic.hip) ---------------------------------------------------------------------------------
def generic_lds_bytes(T, d, n, want_grad, big, dd=False):
    """`generic_lds_bytes`: the per-pair LDS of the coverage kernel.  big: the per-band layout; dd: fp64 increment table"""
    dp = d + 1 if d % 2 == 0 else d
    Tm = T - 1
    TmS, P = Tm | 1, (1 << n) * Tm
    dbl = 2 * T * dp + 2 * T + (P + 2) + 64
    if big:
        return (dbl + 64 * TmS + T) * 8
    flt = Tm * TmS
    if want_grad:
        dbl += Tm * Tm + T * dp
    if dd:
        dbl, flt = dbl + Tm * TmS, 0
    return dbl * 8 + flt * 4


def generic_plan(A, B, T, d, n, want_grad, sym, precise, any_size, cus=256):
    """The launch plan of csrc/gram_generic.hip (`generic_solves_unordered`, `make_plan` and the workspace layout of
    `generic_plan`) for X [A, T, d] x Y [B, T, d] at dyadic order n on `cus` compute units, as a dict: table ("f64": the
    whole-grid increment table in fp64, "f32": in fp32, "big": fp64 increments per band of 64 rows, S in the scratch), lds,
    P, nbands, nsteps, JC, nchunks, items, grid, yx (each unordered pair once), bytes (what sigsvgd_gram_workspace_bytes
    reports for a query that covers this one launch); None where the library refuses the launch (E_UNSUPPORTED).
    `sym`: the Y_IS_X orientation with A == B; `precise`, `any_size`: what the route passes (`generic_route`).
    tests/test_generic_plan_cabi.py pins it to the library."""
    assert A >= 1 and B >= 1 and T >= 2 and d >= 1 and 0 <= n <= 10
    yx = bool(sym) and (any_size or A * B >= 4096)
    if yx and want_grad and A * B * T * d * 8 > (1 << 30):
        yx = False  # the column slab would pass 1 GiB: ordered pairs
    P = (1 << n) * (T - 1)
    if P > 16384:
        return None
    table, lds = "f32", generic_lds_bytes(T, d, n, want_grad, False)
    l2 = generic_lds_bytes(T, d, n, want_grad, False, True)
    if l2 <= (160 if precise else 20) * 1024:
        table, lds = "f64", l2
    elif n == 0 and (precise or lds > 160 * 1024):
        table, lds = "big", generic_lds_bytes(T, d, n, want_grad, True)
    if lds > 160 * 1024:
        return None
    JC = 32
    while JC > 1 and A * -(-B // JC) < (16384 if yx else 2048):
        JC >>= 1
    nchunks = -(-B // JC)
    items = A * nchunks
    grid = min(cus * max(1, min(8, 160 * 1024 // lds)), items)
    nbands, nsteps = -(-P // 64), P + 63
    partial_bytes = A * nchunks * T * d * 8 if want_grad else 0
    col_bytes = (A * B * T * d * 8 + 255) & ~255 if want_grad and yx else 0
    big = table == "big"
    wsk_per_block = nbands * nsteps * 64 * (2 if big else 1) + (64 if big else 0) if want_grad else 0
    return dict(table=table, lds=lds, P=P, nbands=nbands, nsteps=nsteps, JC=JC, nchunks=nchunks, items=items, grid=grid, yx=yx,
                bytes=256 + partial_bytes + col_bytes + wsk_per_block * 4 * grid + 256)


def generic_route(A, B, T, d, n, kind, want_grad, naive=False, force_generic=False, sym=False, cus=256, band_mode=None):
    """`gram_route`'s three ways into the coverage kernel: "Generic", "GenericPrecise", "GenericOneChannel"; None where the
    launch stays on an fp32-sweep family.  kind: the static kernel (0 RBF, 1 linear, 2 IMQ, 3 RQ, 6 / 7 Matern); without
    SIGSVGD_FLAG_FP32_SWEEPS.  -> (route, precise, any_size): the last two are what `generic_plan` takes."""
    if force_generic or kind not in (0, 1):  # (IMQ, RQ, Matern: fp64 kernels only, held to fp64 results)
        return "GenericPrecise", True, False
    fp32 = kind == 0 and not naive
    if fp32 and want_grad and d == 1 and n == 0 and 3 <= T <= 128:
        return "GenericOneChannel", True, True
    if fp32 and gram_geometry(A, B, T, d, n, want_grad, sym, cus, band_mode) is not None:
        return None
    return "Generic", False, False


def routed_generic_plan(A, B, T, d, n, kind, want_grad, naive=False, force_generic=False, sym=False, cus=256):
    """(route, plan) of a Gram call that reaches the coverage kernel (asserted)"""
    r = generic_route(A, B, T, d, n, kind, want_grad, naive, force_generic, sym, cus)
    assert r is not None, "not a launch of the coverage kernel"
    return r[0], generic_plan(A, B, T, d, n, want_grad, sym and A == B, r[1], r[2], cus)


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


def probes(A, B, geom, sym, seed):
    """about 32 pairs (i, j): the first and the last item of twelve workgroup ranges spread over the launch -- a row of the
    item's tile that owns the pair -- and eight random ones"""
    bounds, starts = gram_item_ranges(A, B, geom, sym)
    rows, rng = geom["rows_per_tile"], np.random.default_rng(seed)
    items = [it for w in np.linspace(0, geom["grid"] - 1, 12).astype(int) for it in (bounds[w], bounds[w + 1] - 1)]
    items += list(rng.integers(0, geom["items"], 8))
    out = []
    for k, it in enumerate(items):
        t = int(np.searchsorted(starts, it, side="right")) - 1
        j = int(it - starts[t]) + (t * rows if sym else 0)
        i = min(t * rows + k % rows, A - 1, j if sym else A - 1)
        assert t * rows <= i < A and 0 <= j < B and (not sym or i <= j)
        out.append((i, j))
    return out


# ---- the case matrix of tests/test_gpu_partition.py ----------------------------------------------------------------------
# kernel: the instantiation the shape reaches (gradient launch; `fwd`: what the forward-only launch reaches where it differs).
# T, d, n: path shape and dyadic order; mode: SIGSVGD_BAND_MODE (None: the launcher's own rule).  family / rows: what
# gram_geometry must say of the gradient launch.  AB, N: the ordered and the Y-is-X size of the gradient launch; ABf, Nf: the
# sizes of the forward-only launch where its geometry differs (4-wave workgroups: 4-row tiles for T > 32; three workgroups
# a CU, two for 16 channels) -- None: the forward-only launch has the gradient launch's geometry and runs at its sizes.
# Sizes are the small ragged ones that meet the regime on 256 CUs.  regime "two": the 4-row tiles of gram_dyad.hip exist
# up to 4 * CUs pairs only, so a launch of two or more tiles has fewer than 2 * grid items whatever its shape, and at no
# size does one of its two-item ranges hold a tile boundary (tests/test_gram_geometry.py goes through all of them).  Those
# cases assert what that form can reach: items > grid (workgroups of one and of two items), a range that starts inside a
# tile and a tile met by two workgroups.
PartitionCase = namedtuple("PartitionCase", "kernel T d n mode family rows AB N ABf Nf regime", defaults=(None, None, "full"))
PARTITION_CASES = [
    PartitionCase("fast<4,4,32> LP", 16, 3, 0, None, "fast", 8, (73, 157), 155),
    PartitionCase("fast<8,4,32> LP", 32, 7, 0, None, "fast", 8, (73, 157), 155),
    PartitionCase("fast<8,4,32>", 20, 5, 0, None, "fast", 8, (73, 157), 155),
    PartitionCase("fast<4,8> LP, fwd<4,4>", 64, 3, 0, None, "fast", 8, (43, 97), 93, (53, 117), 109),
    PartitionCase("fast<4,8>, fwd<4,4>", 40, 2, 0, None, "fast", 8, (43, 97), 93, (53, 117), 109),
    PartitionCase("fast<8,8> LP, fwd<8,4>", 64, 7, 0, None, "fast", 8, (43, 97), 93, (53, 117), 109),
    PartitionCase("fast<8,8>, fwd<8,4>", 50, 8, 0, None, "fast", 8, (43, 97), 93, (53, 117), 109),
    PartitionCase("fast<16,4>", 64, 14, 0, None, "fast", 4, (33, 77), 67, (43, 97), 91),
    PartitionCase("fast<16,4>", 33, 9, 0, None, "fast", 4, (33, 77), 67, (43, 97), 91),
    PartitionCase("fast<16,4>", 17, 16, 0, None, "fast", 4, (33, 77), 67, (43, 97), 91),
    PartitionCase("quad<8> early", 100, 7, 0, None, "quad", 8, (43, 97), 93),
    PartitionCase("quad<16>", 128, 14, 0, None, "quad", 8, (43, 97), 93),
    PartitionCase("quad<16> row accumulator", 120, 16, 0, None, "quad", 8, (43, 97), 93),
    PartitionCase("quad<8> early, few-channel fwd", 100, 3, 0, None, "quad", 8, (43, 97), 93),
    PartitionCase("dyad<8,8>, few-channel fwd", 5, 2, 5, "serial", "dyad", 8, (43, 97), 93),
    PartitionCase("dyad<8,8>", 20, 7, 2, "serial", "dyad", 8, (43, 97), 93),
    PartitionCase("dyad<8,4>, few-channel fwd", 5, 2, 5, "serial", "dyad", 4, (9, 113), 44, regime="two"),
    PartitionCase("dyad<8,4>", 20, 7, 2, "serial", "dyad", 4, (9, 113), 44, regime="two"),
    PartitionCase("band<8> serial, 3 bands", 10, 2, 4, "serial", "band serial", 8, (65, 141), 125),
    PartitionCase("band<8> serial, 4 bands", 30, 2, 3, "serial", "band serial", 8, (43, 97), 93),
    PartitionCase("band<16> serial, 3 bands", 18, 14, 3, "serial", "band serial", 8, (43, 97), 93),
    PartitionCase("band<8> parallel, 3 bands", 10, 2, 4, "parallel", "band parallel", 1, (34, 79), 73),
    PartitionCase("band<8> parallel, 4 bands", 30, 2, 3, "parallel", "band parallel", 1, (31, 71), 65),
    PartitionCase("band<16> parallel, 3 bands", 18, 14, 3, "parallel", "band parallel", 1, (34, 79), 73),
]


def case_id(c):
    return f"T{c.T}-d{c.d}-n{c.n}" + (f"-{c.mode}" if c.mode else "") + f"-rows{c.rows}"


def claim_regime(A, B, T, d, n, want_grad, sym, regime, mode=None, cus=None):
    """Print the launch's (family, rows per tile, items, grid) and assert the regime the case claims; -> the geometry"""
    g = gram_geometry(A, B, T, d, n, want_grad, sym, device_cus() if cus is None else cus, mode)
    assert g is not None, "not a launch of the fp32-sweep kernels"
    r = gram_multi_item_regime(A, B, g, sym)
    print(f"{'gradient' if want_grad else 'forward'} {'Y is X' if sym else 'ordered'} {A} x {B}, T={T} d={d} order {n}: "
          f"{g['family']}, {g['rows_per_tile']} rows per tile, {g['items']} items on {g['grid']} workgroups")
    if regime == "two":
        assert g["items"] > g["grid"], g
        r.pop("multi"), r.pop("crosses")
    if regime is not None:
        assert all(r.values()), (g, r)
    return g


def step_scale(n):
    """cumulative sums of steps 0.05 at order 0, 0.3 on refined grids: the regimes the other parity files hold to 1e-5, away
    from the rough few-channel paths that flag pairs for the fp64 pass"""
    return 0.05 if n == 0 else 0.3
