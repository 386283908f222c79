"""GPU parity at the edges of the static work partition of the fp32-sweep Gram kernels (gram_fast.hip, gram_quad.hip,
gram_dyad.hip, gram_band.hip): launches with fewer items than workgroups, one row / one column, row tiles that are not full,
ranges that cross row tiles, and the strided row tiles of the sharded partial solve -- against the fp64 oracle, via the C ABI.

The multi-item regime.  A launch is a list of (row tile, column) items over grid = min(items, resident workgroups)
workgroups, workgroup w taking the items [items*w/grid, items*(w+1)/grid).  With items <= resident every workgroup solves
one column and never loops, prefetches the next column, re-zeroes its per-pair state, starts inside a tile or shares a tile's
row segments with another workgroup.  `plans.PARTITION_CASES` puts every kernel instantiation past that: each case asserts, from
`plans.gram_geometry` with the device's CU count, that items >= 2 grid + 1, that a range starts strictly inside a tile,
that one crosses into the next tile and that a tile is met by two workgroups, and prints (family, rows per tile, items,
grid).  Every row of every launch is compared with the oracle.  tests/test_gram_geometry.py pins `gram_geometry` to the
library and shows on the oracle alone that the gradient metric notices one lost or misfiled pair."""
import numpy as np
import pytest
import torch

from oracle import c_oracle as C
from parity import rel_entry, rel_max, signed_weights, walks
from plans import (case_id, claim_regime, device_cus, gram_geometry,
                   gram_multi_item_regime, PARTITION_CASES, set_band_mode, step_scale)

pytestmark = pytest.mark.gpu

TOL = 1e-5
# two fp32-sweep solves of one pair that differ in orientation (the symmetric launch solves (i, j), the ordered one also
# (j, i)) or launch geometry agree to a few ulps PER ENTRY; both are within TOL of the fp64 oracle
SELF = 4e-6


# ---- the case matrix: plans.PARTITION_CASES (tests/test_gram_geometry.py checks it on 256 compute units) -------------------
# fp64 I/O: one case per family (both band schedules)
IO64 = [c for c in PARTITION_CASES
        if (c.T, c.d, c.n, c.rows) in [(64, 7, 0, 8), (100, 7, 0, 8), (20, 7, 2, 8), (10, 2, 4, 8), (30, 2, 3, 1)]]
# the launch shapes of the register-resident kernel this file held before the matrix: (A, B) at T = 16, d = 3 with normal
# weights and N at T = 12, d = 2 with grad_out = NULL (one row, one column, fewer items than workgroups, a last tile with one
# row); 67 x 263 and N = 257 are in the multi-item regime
EDGE_AB = [(1, 1), (1, 9), (9, 1), (3, 5), (8, 300), (300, 8), (67, 263)]
EDGE_N = [1, 2, 7, 8, 9, 63, 257]


def ordered_params():
    """(A, B, T, d, n, mode, weights, launch, dtype, regime): the edge shapes first (regime None: nothing claimed), then the matrix"""
    out = [pytest.param(A, B, 16, 3, 0, None, "normal", "grad", torch.float32, "full" if (A, B) == (67, 263) else None,
                        id=f"{A}-{B}") for (A, B) in EDGE_AB]
    for c in PARTITION_CASES:
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
    for c in PARTITION_CASES:
        for weights in ("signed", "signed-sym", "ones"):
            out.append(pytest.param(c.N, c.T, c.d, c.n, c.mode, weights, "grad", torch.float32, c.regime,
                                    id=f"{case_id(c)}-{weights}"))
        if c.Nf:
            out.append(pytest.param(c.Nf, c.T, c.d, c.n, c.mode, "ones", "fwd", torch.float32, c.regime, id=case_id(c) + "-fwd"))
    for c in IO64:
        out.append(pytest.param(c.N, c.T, c.d, c.n, c.mode, "signed", "grad", torch.float64, c.regime, id=case_id(c) + "-io64"))
    return out


@pytest.mark.parametrize("A,B,T,d,n,mode,weights,launch,dtype,regime", ordered_params())
def test_ordered_launch_shapes(gpu, monkeypatch, A, B, T, d, n, mode, weights, launch, dtype, regime):
    """X != Y: items = row tiles x all columns, grad_out random and signed.  67 x 263 at T = 16, d = 3 is 9 tiles x 263
    columns = 2,367 items over 768 workgroups (three per CU on the 32-slot ring).  launch "grad": the gradient launch at
    its regime, and the forward-only launch on the same paths; "fwd": the forward-only launch at a size of its own geometry."""
    from sigsvgd_amd import ops

    set_band_mode(monkeypatch, mode)
    h = 0.9
    X, Y = walks(A, T, d, 11, step_scale(n)), walks(B, T, d, 12, step_scale(n))
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
    eKf = rel_entry(Kf.cpu().numpy(), Kref, 1e-6)
    print(f"K forward-only {eKf:.2e}")
    assert Kf.dtype == dtype and eKf < TOL
    if grad:
        eK, eg = rel_entry(K.cpu().numpy(), Kref, 1e-6), rel_max(gx.cpu().numpy(), gref)
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

    set_band_mode(monkeypatch, mode)
    h = 1.1
    X = walks(N, T, d, 21, step_scale(n))
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
    eKf = rel_entry(Kf.cpu().numpy(), Kref, 1e-6)
    print(f"K forward-only {eKf:.2e}")
    assert Kf.dtype == dtype and eKf < TOL
    assert torch.equal(Kf, Kf.T)
    if grad:
        eK, eg = rel_entry(K.cpu().numpy(), Kref, 1e-6), rel_max(gx.cpu().numpy(), gref)
        print(f"K {eK:.2e} gradient {eg:.2e}")
        assert K.dtype == dtype and gx.dtype == dtype
        assert eK < TOL and eg < TOL
        assert torch.equal(K, K.T)
    if grad and go is not None:
        Ko, gxo = ops.gram_fwd_bwd(Xg, Xg.clone(), 1.0 / h, n, grad_out=gog, sym=sym)
        torch.cuda.synchronize()
        eKo, ego = rel_entry(Ko.cpu().numpy(), K.double().cpu().numpy(), 1e-6), rel_max(gxo.cpu().numpy(), gx.double().cpu().numpy())
        print(f"against the ordered launch: K {eKo:.2e} gradient {ego:.2e}")
        assert eKo < SELF and ego < TOL


@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("N,stride,T", [(20, 3, 20), (70, 8, 20), (9, 2, 20), (5, 4, 20), (100, 3, 40), (131, 4, 64)])
def test_partial_shares_sum_to_full(gpu, N, stride, T, fold):
    """Strided row tiles (more ranks than tiles included), cyclic and folded ownership: the shares add up to the symmetric
    solve, every pair belongs to exactly one share, and a share holds exactly the tiles `ops.owned_tiles` lists."""
    from sigsvgd_amd import ops

    d, h = 7, 1.0
    X = walks(N, T, d, 31, 0.05)
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
    assert rel_entry(Ks.cpu().numpy(), K.double().cpu().numpy(), 1e-6) < SELF
    assert rel_max(gs.cpu().numpy(), g.double().cpu().numpy()) < 1e-5


@pytest.mark.parametrize("weights", ["signed", "signed-sym"])
@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("N,T,d", [(251, 20, 5), (155, 64, 7), (149, 64, 14), (155, 100, 7)])
def test_weighted_partial_shares_in_the_multi_item_regime(gpu, N, T, d, fold, weights):
    """The two shares of a partial solve with grad_out (register-resident kernel with 8- and 4-row tiles and on the
    32-slot ring, quadrant kernel), each in the multi-item regime over its own tiles -- strided, and the mirror images in
    descending order when folded: they add up to the weighted symmetric launch (K exactly) and to the oracle."""
    from sigsvgd_amd import ops

    h, stride = 1.0, 2
    X = walks(N, T, d, 31, 0.05)
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
    eK, eg = rel_entry(Ks.cpu().numpy(), Kref, 1e-6), rel_max(gs.cpu().numpy(), gref)
    print(f"K {eK:.2e} gradient {eg:.2e}")
    assert torch.equal(Ks, K)
    assert eK < TOL and eg < TOL
    assert rel_max(gs.cpu().numpy(), g.double().cpu().numpy()) < TOL


def test_partial_solve_refuses_weights_of_another_shape(gpu):
    """The kernel reads N * N weights whatever it is given: `ops.gram_sym_partial` refuses a grad_out that is not [N, N] like
    every other weighted launch, before anything is launched (the caller's `out` buffers keep what they held)."""
    from sigsvgd_amd import ops

    N, T, d = 8, 8, 2
    Xg = torch.as_tensor(walks(N, T, d, 31, 0.05), device=gpu)
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
    X, Y = walks(A, 136, d, 41, scale=0.03), walks(B, 136, d, 42, scale=0.03)
    Kref, gref = C.gram_fwd_bwd(X, Y, h, 0)
    K, g = ops.gram_fwd_bwd(torch.as_tensor(X, device=gpu), torch.as_tensor(Y, device=gpu), 1.0 / h)
    Ksr, gsr = C.gram_fwd_bwd(X, X, h, 0)
    Xg = torch.as_tensor(X, device=gpu)
    Ks, gs = ops.gram_fwd_bwd(Xg, Xg, 1.0 / h, y_is_x=True)
    torch.cuda.synchronize()
    assert rel_entry(K.cpu().numpy(), Kref, 1e-6) < TOL and rel_max(g.cpu().numpy(), gref) < TOL
    assert rel_entry(Ks.cpu().numpy(), Ksr, 1e-6) < TOL and rel_max(gs.cpu().numpy(), gsr) < TOL

    X2, Y2 = walks(3, 190, d, 43, scale=0.03), walks(4, 190, d, 44, scale=0.03)
    Kref2, gref2 = C.gram_fwd_bwd(X2, Y2, h, 0)
    X2g, Y2g = torch.as_tensor(X2, device=gpu), torch.as_tensor(Y2, device=gpu)
    K2 = ops.gram_fwd(X2g, Y2g, 1.0 / h)
    assert rel_entry(K2.cpu().numpy(), Kref2, 1e-6) < TOL
    K3, g3 = ops.gram_fwd_bwd(X2g, Y2g, 1.0 / h)
    assert rel_entry(K3.cpu().numpy(), Kref2, 1e-6) < TOL and rel_max(g3.cpu().numpy(), gref2) < TOL
    X4 = torch.as_tensor(walks(3, 300, d, 45, scale=0.03), device=gpu)
    with pytest.raises(RuntimeError, match="LDS"):
        ops.gram_fwd_bwd(X4, X4.clone(), 1.0 / h)
    with pytest.raises(RuntimeError, match="LDS"):
        ops.gram_fwd(X4, X4.clone(), 1.0 / h)
