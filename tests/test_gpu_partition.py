"""GPU parity at the edges of the static work partition of the fp32-sweep Gram kernels (gram_fast.hip, gram_quad.hip,
gram_dyad.hip, gram_band.hip): launches with fewer items than workgroups, one row / one column, row tiles that are not full,
ranges that cross row tiles, and the strided row tiles of the sharded partial solve -- against the fp64 oracle, via the C ABI.

The multi-item regime.  A launch is a list of (row tile, column) items over grid = min(items, resident workgroups)
workgroups, workgroup w taking the items [items*w/grid, items*(w+1)/grid).  With items <= resident every workgroup solves
one column and never loops, prefetches the next column, re-zeroes its per-pair state, starts inside a tile or shares a tile's
row segments with another workgroup.  CASES below puts every kernel instantiation past that: each case asserts, from
`helpers.gram_geometry` with the device's CU count, that items >= 2 grid + 1, that a range starts strictly inside a tile,
that one crosses into the next tile and that a tile is met by two workgroups, and prints (family, rows per tile, items,
grid).  Every row of every launch is compared with the oracle.  tests/test_gram_geometry.py pins `gram_geometry` to the
library and shows on the oracle alone that the gradient metric notices one lost or misfiled pair."""
from collections import namedtuple

import numpy as np
import pytest
import torch

from helpers import device_cus, gram_geometry, gram_multi_item_regime, signed_weights
from oracle import c_oracle as C

pytestmark = pytest.mark.gpu

TOL = 1e-5
# two fp32-sweep solves of one pair that differ in orientation (the symmetric launch solves (i, j), the ordered one also
# (j, i)) or launch geometry agree to a few ulps PER ENTRY; both are within TOL of the fp64 oracle
SELF = 4e-6


def _paths(A, T, d, seed, scale=0.05):
    rng = np.random.default_rng(seed)
    return np.cumsum(scale * rng.standard_normal((A, T, d)), axis=1).astype(np.float32)


def _rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-300))


def _relK(a, b):
    """K parity as north_star states it: max over entries of |K - K_ref| / |K_ref| (K > 0 always)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    # (round 4: plain relative error per entry -- rounds 2-3 floored the denominator at 0.1; the 1e-6 only keeps an exact zero
    #  out of it.  Pairs whose K is small against their grid are solved by the exact fp64 pass now: DESIGN.md section 3)
    return float((np.abs(a - b) / np.maximum(np.abs(b), 1e-6)).max())


# ---- the case matrix ------------------------------------------------------------------------------------------------------
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
Case = namedtuple("Case", "kernel T d n mode family rows AB N ABf Nf regime", defaults=(None, None, "full"))
CASES = [
    Case("fast<4,4,32> LP", 16, 3, 0, None, "fast", 8, (73, 157), 155),
    Case("fast<8,4,32> LP", 32, 7, 0, None, "fast", 8, (73, 157), 155),
    Case("fast<8,4,32>", 20, 5, 0, None, "fast", 8, (73, 157), 155),
    Case("fast<4,8> LP, fwd<4,4>", 64, 3, 0, None, "fast", 8, (43, 97), 93, (53, 117), 109),
    Case("fast<4,8>, fwd<4,4>", 40, 2, 0, None, "fast", 8, (43, 97), 93, (53, 117), 109),
    Case("fast<8,8> LP, fwd<8,4>", 64, 7, 0, None, "fast", 8, (43, 97), 93, (53, 117), 109),
    Case("fast<8,8>, fwd<8,4>", 50, 8, 0, None, "fast", 8, (43, 97), 93, (53, 117), 109),
    Case("fast<16,4>", 64, 14, 0, None, "fast", 4, (33, 77), 67, (43, 97), 91),
    Case("fast<16,4>", 33, 9, 0, None, "fast", 4, (33, 77), 67, (43, 97), 91),
    Case("fast<16,4>", 17, 16, 0, None, "fast", 4, (33, 77), 67, (43, 97), 91),
    Case("quad<8> early", 100, 7, 0, None, "quad", 8, (43, 97), 93),
    Case("quad<16>", 128, 14, 0, None, "quad", 8, (43, 97), 93),
    Case("quad<16> row accumulator", 120, 16, 0, None, "quad", 8, (43, 97), 93),
    Case("quad<8> early, few-channel fwd", 100, 3, 0, None, "quad", 8, (43, 97), 93),
    Case("dyad<8,8>, few-channel fwd", 5, 2, 5, "serial", "dyad", 8, (43, 97), 93),
    Case("dyad<8,8>", 20, 7, 2, "serial", "dyad", 8, (43, 97), 93),
    Case("dyad<8,4>, few-channel fwd", 5, 2, 5, "serial", "dyad", 4, (9, 113), 44, regime="two"),
    Case("dyad<8,4>", 20, 7, 2, "serial", "dyad", 4, (9, 113), 44, regime="two"),
    Case("band<8> serial, 3 bands", 10, 2, 4, "serial", "band serial", 8, (65, 141), 125),
    Case("band<8> serial, 4 bands", 30, 2, 3, "serial", "band serial", 8, (43, 97), 93),
    Case("band<16> serial, 3 bands", 18, 14, 3, "serial", "band serial", 8, (43, 97), 93),
    Case("band<8> parallel, 3 bands", 10, 2, 4, "parallel", "band parallel", 1, (34, 79), 73),
    Case("band<8> parallel, 4 bands", 30, 2, 3, "parallel", "band parallel", 1, (31, 71), 65),
    Case("band<16> parallel, 3 bands", 18, 14, 3, "parallel", "band parallel", 1, (34, 79), 73),
]
# fp64 I/O: one case per family (both band schedules)
IO64 = [c for c in CASES if (c.T, c.d, c.n, c.rows) in [(64, 7, 0, 8), (100, 7, 0, 8), (20, 7, 2, 8), (10, 2, 4, 8), (30, 2, 3, 1)]]
# the launch shapes of the register-resident kernel this file held before the matrix: (A, B) at T = 16, d = 3 with normal
# weights and N at T = 12, d = 2 with grad_out = NULL (one row, one column, fewer items than workgroups, a last tile with one
# row); 67 x 263 and N = 257 are in the multi-item regime
EDGE_AB = [(1, 1), (1, 9), (9, 1), (3, 5), (8, 300), (300, 8), (67, 263)]
EDGE_N = [1, 2, 7, 8, 9, 63, 257]


def case_id(c):
    return f"T{c.T}-d{c.d}-n{c.n}" + (f"-{c.mode}" if c.mode else "") + f"-rows{c.rows}"


def ordered_params():
    """(A, B, T, d, n, mode, weights, launch, dtype, regime): the edge shapes first (regime None: nothing claimed), then CASES"""
    out = [pytest.param(A, B, 16, 3, 0, None, "normal", "grad", torch.float32, "full" if (A, B) == (67, 263) else None,
                        id=f"{A}-{B}") for (A, B) in EDGE_AB]
    for c in CASES:
        out.append(pytest.param(*c.AB, c.T, c.d, c.n, c.mode, "signed", "grad", torch.float32, c.regime, id=case_id(c)))
        if c.ABf:
            out.append(pytest.param(*c.ABf, c.T, c.d, c.n, c.mode, "signed", "fwd", torch.float32, c.regime, id=case_id(c) + "-fwd"))
    for c in IO64:
        out.append(pytest.param(*c.AB, c.T, c.d, c.n, c.mode, "signed", "grad", torch.float64, c.regime, id=case_id(c) + "-io64"))
    return out


def symmetric_params():
    """(N, T, d, n, mode, weights, launch, dtype, regime)"""
    out = [pytest.param(N, 12, 2, 0, None, "ones", "grad", torch.float32, "full" if N == 257 else None, id=str(N))
           for N in EDGE_N]
    for c in CASES:
        for weights in ("signed", "signed-sym", "ones"):
            out.append(pytest.param(c.N, c.T, c.d, c.n, c.mode, weights, "grad", torch.float32, c.regime,
                                    id=f"{case_id(c)}-{weights}"))
        if c.Nf:
            out.append(pytest.param(c.Nf, c.T, c.d, c.n, c.mode, "ones", "fwd", torch.float32, c.regime, id=case_id(c) + "-fwd"))
    for c in IO64:
        out.append(pytest.param(c.N, c.T, c.d, c.n, c.mode, "signed", "grad", torch.float64, c.regime, id=case_id(c) + "-io64"))
    return out


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


def _set_mode(monkeypatch, mode):
    if mode is None:
        monkeypatch.delenv("SIGSVGD_BAND_MODE", raising=False)
    else:
        monkeypatch.setenv("SIGSVGD_BAND_MODE", mode)


def step_scale(n):
    """cumulative sums of steps 0.05 at order 0, 0.3 on refined grids: the regimes the other parity files hold to 1e-5, away
    from the rough few-channel paths that flag pairs for the fp64 pass"""
    return 0.05 if n == 0 else 0.3


@pytest.mark.parametrize("A,B,T,d,n,mode,weights,launch,dtype,regime", ordered_params())
def test_ordered_launch_shapes(gpu, monkeypatch, A, B, T, d, n, mode, weights, launch, dtype, regime):
    """X != Y: items = row tiles x all columns, grad_out random and signed.  67 x 263 at T = 16, d = 3 is 9 tiles x 263
    columns = 2,367 items over 768 workgroups (three per CU on the 32-slot ring).  launch "grad": the gradient launch at
    its regime, and the forward-only launch on the same paths; "fwd": the forward-only launch at a size of its own geometry."""
    from sigsvgd_amd import ops

    _set_mode(monkeypatch, mode)
    h = 0.9
    X, Y = _paths(A, T, d, 11, step_scale(n)), _paths(B, T, d, 12, step_scale(n))
    grad = launch == "grad"
    g = claim_regime(A, B, T, d, n, grad, False, regime)
    gf = gram_geometry(A, B, T, d, n, False, False, device_cus())
    if grad and (gf["rows_per_tile"], gf["grid"]) == (g["rows_per_tile"], g["grid"]):
        claim_regime(A, B, T, d, n, False, False, regime)  # the forward-only launch splits the same way: the same claim
    go = np.random.default_rng(13).standard_normal((A, B)) if weights == "normal" else signed_weights(A, B, 13)
    Kref, gref = C.gram_fwd_bwd(X, Y, h, n, grad_out=go, want_grad=grad)
    Xg, Yg = torch.as_tensor(X, device=gpu).to(dtype), torch.as_tensor(Y, device=gpu).to(dtype)
    if grad:
        K, gx = ops.gram_fwd_bwd(Xg, Yg, 1.0 / h, n, grad_out=torch.as_tensor(go, device=gpu, dtype=dtype))
    Kf = ops.gram_fwd(Xg, Yg, 1.0 / h, n)
    torch.cuda.synchronize()
    eKf = _relK(Kf.cpu().numpy(), Kref)
    print(f"K forward-only {eKf:.2e}")
    assert Kf.dtype == dtype and eKf < TOL
    if grad:
        eK, eg = _relK(K.cpu().numpy(), Kref), _rel(gx.cpu().numpy(), gref)
        print(f"K {eK:.2e} gradient {eg:.2e}")
        assert K.dtype == dtype and gx.dtype == dtype
        assert eK < TOL and eg < TOL


@pytest.mark.parametrize("N,T,d,n,mode,weights,launch,dtype,regime", symmetric_params())
def test_symmetric_launch_shapes(gpu, monkeypatch, N, T, d, n, mode, weights, launch, dtype, regime):
    """Y is X: items = columns from the tile's first row on; N = 257 leaves a last tile with one row.  weights "signed":
    random asymmetric grad_out -- row i takes w_ij from pair (i, j), row j takes w_ji from the same solve --, "signed-sym":
    the same with SIGSVGD_FLAG_SYM (w_ij + w_ji both ways), "ones": grad_out = NULL.  The weighted launches also equal the
    ordered launch on (X, X.clone()) with the same weights, which ties the two decodes to each other."""
    from sigsvgd_amd import ops

    _set_mode(monkeypatch, mode)
    h = 1.1
    X = _paths(N, T, d, 21, step_scale(n))
    grad = launch == "grad"
    g = claim_regime(N, N, T, d, n, grad, True, regime)
    gf = gram_geometry(N, N, T, d, n, False, True, device_cus())
    if grad and (gf["rows_per_tile"], gf["grid"]) == (g["rows_per_tile"], g["grid"]):
        claim_regime(N, N, T, d, n, False, True, regime)
    go = None if weights == "ones" else signed_weights(N, N, 23)
    sym = weights == "signed-sym"
    # first-slot gradient; Y is X only says each unordered pair is solved once
    Kref, gref = C.gram_fwd_bwd(X, X, h, n, grad_out=go + go.T if sym else go, want_grad=grad)
    Xg = torch.as_tensor(X, device=gpu).to(dtype)
    gog = None if go is None else torch.as_tensor(go, device=gpu, dtype=dtype)
    if grad:
        K, gx = ops.gram_fwd_bwd(Xg, Xg, 1.0 / h, n, grad_out=gog, sym=sym, y_is_x=True)
    Kf = ops.gram_fwd(Xg, Xg, 1.0 / h, n, y_is_x=True)
    torch.cuda.synchronize()
    eKf = _relK(Kf.cpu().numpy(), Kref)
    print(f"K forward-only {eKf:.2e}")
    assert Kf.dtype == dtype and eKf < TOL
    assert torch.equal(Kf, Kf.T)
    if grad:
        eK, eg = _relK(K.cpu().numpy(), Kref), _rel(gx.cpu().numpy(), gref)
        print(f"K {eK:.2e} gradient {eg:.2e}")
        assert K.dtype == dtype and gx.dtype == dtype
        assert eK < TOL and eg < TOL
        assert torch.equal(K, K.T)
    if grad and go is not None:
        Ko, gxo = ops.gram_fwd_bwd(Xg, Xg.clone(), 1.0 / h, n, grad_out=gog, sym=sym)
        torch.cuda.synchronize()
        eKo, ego = _relK(Ko.cpu().numpy(), K.double().cpu().numpy()), _rel(gxo.cpu().numpy(), gx.double().cpu().numpy())
        print(f"against the ordered launch: K {eKo:.2e} gradient {ego:.2e}")
        assert eKo < SELF and ego < TOL


@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("N,stride,T", [(20, 3, 20), (70, 8, 20), (9, 2, 20), (5, 4, 20), (100, 3, 40), (131, 4, 64)])
def test_partial_shares_sum_to_full(gpu, N, stride, T, fold):
    """Strided row tiles (more ranks than tiles included), cyclic and folded ownership: the shares add up to the symmetric
    solve, every pair belongs to exactly one share, and a share holds exactly the tiles `ops.owned_tiles` lists."""
    from sigsvgd_amd import ops

    d, h = 7, 1.0
    X = _paths(N, T, d, 31)
    Xg = torch.as_tensor(X, device=gpu)
    K, g = ops.gram_fwd_bwd(Xg, Xg, 1.0 / h, y_is_x=True)
    Ks = torch.zeros_like(K)
    gs = torch.zeros(N, T, d, device=gpu, dtype=torch.float64)
    nw = ops.sym_tile_rows(T, d)
    ntile = (N + nw - 1) // nw
    for r in range(stride):
        Kp, gp = ops.gram_sym_partial(Xg, 1.0 / h, r, stride, fold=fold)
        Ks += Kp
        gs += gp
        # upper-triangle rows with an entry right of the diagonal are the rows of the owned tiles
        up = torch.triu(Kp != 0)
        rows = set(int(i) // nw for i in torch.nonzero(up.any(dim=1)).flatten().tolist())
        assert rows == set(ops.owned_tiles(ntile, r, stride, fold)), (r, rows)
    torch.cuda.synchronize()
    assert torch.equal(Ks, K)
    assert _relK(Ks.cpu().numpy(), K.double().cpu().numpy()) < SELF
    assert _rel(gs.cpu().numpy(), g.double().cpu().numpy()) < 1e-5


@pytest.mark.parametrize("weights", ["signed", "signed-sym"])
@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("N,T,d", [(251, 20, 5), (155, 64, 7), (149, 64, 14), (155, 100, 7)])
def test_weighted_partial_shares_in_the_multi_item_regime(gpu, N, T, d, fold, weights):
    """The two shares of a partial solve with grad_out (register-resident kernel with 8- and 4-row tiles and on the
    32-slot ring, quadrant kernel), each in the multi-item regime over its own tiles -- strided, and the mirror images in
    descending order when folded: they add up to the weighted symmetric launch (K exactly) and to the oracle."""
    from sigsvgd_amd import ops

    h, stride = 1.0, 2
    X = _paths(N, T, d, 31)
    go, sym = signed_weights(N, N, 33), weights == "signed-sym"
    Kref, gref = C.gram_fwd_bwd(X, X, h, 0, grad_out=go + go.T if sym else go)
    Xg, gog = torch.as_tensor(X, device=gpu), torch.as_tensor(go, device=gpu, dtype=torch.float32)
    K, g = ops.gram_fwd_bwd(Xg, Xg, 1.0 / h, grad_out=gog, sym=sym, y_is_x=True)
    full = gram_geometry(N, N, T, d, 0, True, True, device_cus())
    nw = ops.sym_tile_rows(T, d)
    assert nw == full["rows_per_tile"]
    Ks = torch.zeros_like(K)
    gs = torch.zeros(N, T, d, device=gpu, dtype=torch.float64)
    for r in range(stride):
        tiles = ops.owned_tiles((N + nw - 1) // nw, r, stride, fold)
        items = sum(N - t * nw for t in tiles)
        share = dict(rows_per_tile=nw, items=items, grid=min(items, full["resident"]))
        print(f"share {r} of {stride}{' folded' if fold else ''}, N={N} T={T} d={d}: {full['family']}, {nw} rows per tile, "
              f"{len(tiles)} tiles, {items} items on {share['grid']} workgroups")
        regime = gram_multi_item_regime(N, N, share, True, tiles)
        assert all(regime.values()), (share, regime)
        Kp, gp = ops.gram_sym_partial(Xg, 1.0 / h, r, stride, grad_out=gog, sym=sym, fold=fold)
        Ks += Kp
        gs += gp
    torch.cuda.synchronize()
    eK, eg = _relK(Ks.cpu().numpy(), Kref), _rel(gs.cpu().numpy(), gref)
    print(f"K {eK:.2e} gradient {eg:.2e}")
    assert torch.equal(Ks, K)
    assert eK < TOL and eg < TOL
    assert _rel(gs.cpu().numpy(), g.double().cpu().numpy()) < TOL


def test_partial_solve_refuses_weights_of_another_shape(gpu):
    """The kernel reads N * N weights whatever it is given: `ops.gram_sym_partial` refuses a grad_out that is not [N, N] like
    every other weighted launch, before anything is launched (the caller's `out` buffers keep what they held)."""
    from sigsvgd_amd import ops

    N, T, d = 8, 8, 2
    Xg = torch.as_tensor(_paths(N, T, d, 31), device=gpu)
    Kp = torch.full((N, N), 7.0, device=gpu, dtype=Xg.dtype)
    gp = torch.full((N, T, d), 7.0, device=gpu, dtype=torch.float64)
    with pytest.raises(ValueError, match="grad_out must be"):
        ops.gram_sym_partial(Xg, 1.0, 0, 1, grad_out=torch.ones(N, N - 1, device=gpu, dtype=Xg.dtype), out=(Kp, gp))
    assert bool((Kp == 7.0).all()) and bool((gp == 7.0).all())


def test_paths_beyond_128_points(gpu):
    """T > 128 (dyadic order 0) is the coverage kernel's: its long-path layout (fp64 increments per band of 64 rows, S in the
    launch's scratch; round 4) takes paths while 64 (T-1) + 2 T d doubles fit 160 KB of LDS -- T = 190 with the gradient,
    which round 3 refused --, longer ones are refused loudly."""
    from sigsvgd_amd import ops

    A, B, h, d = 5, 4, 1.2, 2
    X, Y = _paths(A, 136, d, 41, scale=0.03), _paths(B, 136, d, 42, scale=0.03)
    Kref, gref = C.gram_fwd_bwd(X, Y, h, 0)
    K, g = ops.gram_fwd_bwd(torch.as_tensor(X, device=gpu), torch.as_tensor(Y, device=gpu), 1.0 / h)
    Ksr, gsr = C.gram_fwd_bwd(X, X, h, 0)
    Xg = torch.as_tensor(X, device=gpu)
    Ks, gs = ops.gram_fwd_bwd(Xg, Xg, 1.0 / h, y_is_x=True)
    torch.cuda.synchronize()
    assert _relK(K.cpu().numpy(), Kref) < TOL and _rel(g.cpu().numpy(), gref) < TOL
    assert _relK(Ks.cpu().numpy(), Ksr) < TOL and _rel(gs.cpu().numpy(), gsr) < TOL

    X2, Y2 = _paths(3, 190, d, 43, scale=0.03), _paths(4, 190, d, 44, scale=0.03)
    Kref2, gref2 = C.gram_fwd_bwd(X2, Y2, h, 0)
    X2g, Y2g = torch.as_tensor(X2, device=gpu), torch.as_tensor(Y2, device=gpu)
    K2 = ops.gram_fwd(X2g, Y2g, 1.0 / h)
    assert _relK(K2.cpu().numpy(), Kref2) < TOL
    K3, g3 = ops.gram_fwd_bwd(X2g, Y2g, 1.0 / h)
    assert _relK(K3.cpu().numpy(), Kref2) < TOL and _rel(g3.cpu().numpy(), gref2) < TOL
    X4 = torch.as_tensor(_paths(3, 300, d, 45, scale=0.03), device=gpu)
    with pytest.raises(RuntimeError, match="LDS"):
        ops.gram_fwd_bwd(X4, X4.clone(), 1.0 / h)
    with pytest.raises(RuntimeError, match="LDS"):
        ops.gram_fwd(X4, X4.clone(), 1.0 / h)
