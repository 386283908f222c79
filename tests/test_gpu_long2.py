"""The two-sided long-path Gram launch (csrc/gram_long.hip `gram_long2_kernel`, `ops.gram_long_fwd_bwd2`, DESIGN.md section
5.12) and what `sigsvgd_amd.sigkernel` builds on it: gradients for both slots of compute_Gram / compute_mmd (`grad_Y`), and
Y = X launches that solve each unordered pair once.  Against the C oracle (fp64).  The oracle differentiates the first slot
only; the second slot's reference is the first slot of the swapped call, d2 k(X, Y) = d1 k(Y, X) with grad_out transposed
(tests/test_long2_cabi.py checks that identity on the numpy oracle).  Tolerances are the long route's own
(tests/test_gpu_long.py): K within 1e-9 per entry with fp64 I/O and within 2^-23 with fp32 I/O, each gradient within 1e-5 of
its own largest entry."""
import numpy as np
import pytest
import torch

from oracle import c_oracle
from parity import DisguisedRBF, np64, rel_entry, rel_max, sized_walks
from plans import BRANCH_CASES, branch_id, branch_regime, device_cus, long2_plan, oracle_at_own_lengths

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32


def oracle_both_slots(X, Y, h, n, naive, kind, W, nthreads=0):
    """(K, gX, gY) of sum W * K(X, Y) from the C oracle, each batch at its own length: gY is the first slot of the swapped
    call with W^T (the padded batch's gradient folded back onto its points by `oracle_at_own_lengths`)."""
    W = np.ones((X.shape[0], Y.shape[0])) if W is None else W
    Kr, gXr = oracle_at_own_lengths(X, Y, h, n, naive, kind, W, nthreads)
    _, gYr = oracle_at_own_lengths(Y, X, h, n, naive, kind, np.ascontiguousarray(W.T), nthreads)
    return Kr, gXr, gYr


def check_two_slot(gpu, X, Y, h, n, kind, naive, io, W, nthreads=0):
    """one two-slot launch against the oracle, the same bits from each output alone, from a second call and for K from the
    ordered forward launch"""
    from sigsvgd_amd import ops

    Kr, gXr, gYr = oracle_both_slots(X, Y, h, n, naive, kind, W, nthreads)
    Xt, Yt = torch.as_tensor(X, dtype=io, device=gpu), torch.as_tensor(Y, dtype=io, device=gpu)
    Wt = None if W is None else torch.as_tensor(W, device=gpu)
    K, gX, gY = ops.gram_long_fwd_bwd2(Xt, Yt, 1.0 / h, n, kind, Wt, naive)
    assert K.shape == Kr.shape and gX.shape == Xt.shape and gY.shape == Yt.shape
    assert K.dtype == gX.dtype == gY.dtype == io
    eK, eX, eY = rel_entry(np64(K), Kr, 0.0), rel_max(np64(gX), gXr), rel_max(np64(gY), gYr)
    print(f"two-slot K {eK:.3e} gX {eX:.3e} gY {eY:.3e}")
    assert eK < (1e-9 if io == F64 else 2.0**-23)
    assert eX < 1e-5
    assert eY < 1e-5
    assert torch.equal(ops.gram_long_fwd(Xt, Yt, 1.0 / h, n, kind, naive), K)
    Kx, gx, none_y = ops.gram_long_fwd_bwd2(Xt, Yt, 1.0 / h, n, kind, Wt, naive, want_gradY=False)
    Ky, none_x, gy = ops.gram_long_fwd_bwd2(Xt, Yt, 1.0 / h, n, kind, Wt, naive, want_gradX=False)
    assert none_x is None and none_y is None
    assert torch.equal(Kx, K) and torch.equal(Ky, K) and torch.equal(gx, gX) and torch.equal(gy, gY)
    K2, gX2, gY2 = ops.gram_long_fwd_bwd2(Xt, Yt, 1.0 / h, n, kind, Wt, naive)
    assert torch.equal(K2, K) and torch.equal(gX2, gX) and torch.equal(gY2, gY)
    K0 = ops.gram_long_fwd_bwd2(Xt, Yt, 1.0 / h, n, kind, None, naive, want_gradX=False, want_gradY=False)[0]
    assert torch.equal(K0, K)


# ---- the two-slot launch ---------------------------------------------------------------------------------------------------
# (A, B, TX, TY, d, n, kind, naive, io, weights): RBF and linear, both stencils, both I/O types, unit and random weights,
# TX != TY, orders 0 and 2, more than one band (TX > 65)
CASES = [
    (3, 4, 300, 300, 3, 0, 0, False, F64, "rand"),
    (3, 4, 300, 300, 3, 0, 0, False, F32, "ones"),
    (2, 3, 1024, 1024, 2, 0, 0, False, F64, "ones"),
    (2, 2, 200, 200, 4, 2, 0, False, F64, "rand"),
    (2, 2, 300, 300, 2, 0, 0, True, F64, "ones"),
    (3, 3, 257, 257, 5, 0, 1, False, F64, "rand"),
    (3, 2, 100, 70, 2, 2, 1, True, F32, "rand"),
    (3, 4, 400, 150, 2, 0, 0, False, F64, "rand"),
    (4, 3, 150, 400, 2, 0, 0, False, F32, "rand"),
]


@pytest.mark.parametrize("A,B,TX,TY,d,n,kind,naive,io,weights", CASES)
def test_two_slot_matches_oracle(gpu, A, B, TX, TY, d, n, kind, naive, io, weights):
    rng = np.random.default_rng(A * 100 + TX + TY + n + kind)
    X, Y = sized_walks(rng, A, TX, d), sized_walks(rng, B, TY, d)
    W = rng.uniform(0.5, 1.5, (A, B)) if weights == "rand" else None
    check_two_slot(gpu, X, Y, 0.5, n, kind, naive, io, W)


@pytest.mark.parametrize("A,B,TX,TY,d,n,kind,naive,regime", BRANCH_CASES, ids=[branch_id(c) for c in BRANCH_CASES])
def test_two_slot_plan_branches(gpu, A, B, TX, TY, d, n, kind, naive, regime):
    """The regimes of test_gpu_long.py's plan-branch test (ring full / wrapping, nrow = 1, one-row last band, single coarse
    row or column, unequal lengths, channels past 16), now with the column side."""
    pl = long2_plan(A, B, TX, TY, d, n, True, True, False, device_cus())
    assert pl is not None and branch_regime(regime, pl, TX, TY), pl
    rng = np.random.default_rng(TX * 7 + TY + 100 * d + n + 13 * kind)
    X, Y = sized_walks(rng, A, TX, d, d**-0.5), sized_walks(rng, B, TY, d, d**-0.5)
    W = rng.uniform(0.5, 1.5, (A, B))
    check_two_slot(gpu, X, Y, 0.5, n, kind, naive, F64, W, nthreads=2 if max(pl["P"], pl["Q"]) > 4096 else 0)


# (A, B, TX, TY, io): tiles of several pairs in both directions with ragged last chunks, more items than resident waves
TILE_CASES = [(210, 330, 12, 16, F64), (150, 250, 16, 20, F32), (5, 70, 40, 40, F64), (131, 151, 20, 20, F64)]


@pytest.mark.parametrize("A,B,TX,TY,io", TILE_CASES)
def test_two_slot_tiles(gpu, A, B, TX, TY, io):
    pl = long2_plan(A, B, TX, TY, 2, 0, True, True, False, device_cus())
    if (A, B) == (5, 70):  # few pairs: one pair per item, every column slab reduced over 5 tile rows
        assert pl["IC"] == pl["JC"] == 1 and pl["items"] == 350, pl
    else:  # several pairs per item both ways, ragged last tiles, a grid-stride loop
        assert pl["IC"] > 1 and pl["JC"] > 1 and A % pl["IC"] and B % pl["JC"] and pl["items"] > pl["grid"], pl
    rng = np.random.default_rng(A + B)
    X, Y = sized_walks(rng, A, TX, 2), sized_walks(rng, B, TY, 2)
    check_two_slot(gpu, X, Y, 0.5, 0, 0, False, io, rng.uniform(0.5, 1.5, (A, B)))


# ---- the Y-is-X launch -----------------------------------------------------------------------------------------------------
# (A, T, d, n, kind, naive, io): A = 1, 2, not a multiple of the tile, beyond one tile row (tiles of 4: asserted below)
YX_CASES = [
    (1, 300, 2, 0, 0, False, F64),
    (2, 300, 3, 0, 0, False, F64),
    (5, 257, 2, 0, 1, False, F64),
    (7, 130, 2, 0, 0, True, F64),
    (4, 200, 4, 2, 0, False, F64),
    (6, 300, 3, 0, 0, False, F32),
    (262, 16, 2, 0, 0, False, F64),
    (262, 16, 2, 0, 1, False, F32),
]


@pytest.mark.parametrize("A,T,d,n,kind,naive,io", YX_CASES)
def test_y_is_x_matches_oracle(gpu, A, T, d, n, kind, naive, io):
    from sigsvgd_amd import ops

    pl = long2_plan(A, A, T, T, d, n, True, False, True, device_cus())
    if A == 262:
        assert pl["IC"] > 1 and A % pl["IC"] and pl["nti"] > 1 and pl["items"] > pl["grid"], pl
    rng = np.random.default_rng(A * 10 + T + n + kind)
    h = 0.5
    X = sized_walks(rng, A, T, d)
    Xt = torch.as_tensor(X, dtype=io, device=gpu)
    Kf = ops.gram_long_fwd(Xt, Xt, 1.0 / h, n, kind, naive)
    iu = torch.triu_indices(A, A, device=gpu)
    W = rng.uniform(0.5, 1.5, (A, A))  # (not symmetric)
    for (weights, sym) in [(None, False), (W, False), (W, True), (None, True)]:
        Wref = np.ones((A, A)) if weights is None else weights
        Kr, gr = c_oracle.gram_fwd_bwd(X, X, h=h, n=n, naive=naive, kind=kind, grad_out=Wref + Wref.T if sym else Wref)
        Wt = None if weights is None else torch.as_tensor(weights, device=gpu)
        K, gX, none_y = ops.gram_long_fwd_bwd2(Xt, Xt, 1.0 / h, n, kind, Wt, naive, sym=sym, y_is_x=True)
        assert none_y is None and K.dtype == gX.dtype == io and gX.shape == Xt.shape
        assert torch.equal(K[iu[0], iu[1]], Kf[iu[0], iu[1]])  # the upper triangle and diagonal keep the ordered launch's bits
        assert torch.equal(K, K.T)
        eK, eX = rel_entry(np64(K), Kr, 0.0), rel_max(np64(gX), gr)
        print(f"y-is-x sym={sym} weighted={weights is not None} K {eK:.3e} gX {eX:.3e}")
        assert eK < (1e-9 if io == F64 else 2.0**-23)
        assert eX < 1e-5
        K2, gX2, _ = ops.gram_long_fwd_bwd2(Xt, Xt.clone(), 1.0 / h, n, kind, Wt, naive, sym=sym, y_is_x=True)
        assert torch.equal(K2, K) and torch.equal(gX2, gX)  # the same bits again, and from a second buffer of equal values
    K0 = ops.gram_long_fwd_bwd2(Xt, Xt, 1.0 / h, n, kind, None, naive, y_is_x=True, want_gradX=False, want_gradY=False)[0]
    assert torch.equal(K0, K)


def test_y_is_x_agrees_with_ordered_launch(gpu):
    from sigsvgd_amd import ops

    rng = np.random.default_rng(4)
    X = torch.as_tensor(sized_walks(rng, 9, 300, 3), dtype=F64, device=gpu)
    W = torch.as_tensor(rng.standard_normal((9, 9)), device=gpu)
    Ko, go = ops.gram_long_fwd_bwd(X, X, 2.0, 0, 0, W)
    K, g, _ = ops.gram_long_fwd_bwd2(X, X, 2.0, 0, 0, W, y_is_x=True)
    assert rel_entry(np64(K), np64(Ko), 0.0) < 1e-9 and rel_max(np64(g), np64(go)) < 1e-9


# ---- the autograd surface --------------------------------------------------------------------------------------------------
def _leafs(gpu, A, B, TX, TY, d, seed, dtype=F64):
    rng = np.random.default_rng(seed)
    Xn, Yn = sized_walks(rng, A, TX, d), sized_walks(rng, B, TY, d)
    X = torch.as_tensor(Xn, dtype=dtype, device=gpu).requires_grad_(True)
    Y = torch.as_tensor(Yn, dtype=dtype, device=gpu).requires_grad_(True)
    return Xn, Yn, X, Y, rng


# long: refused by the fused kernels; fused: T = 16, d = 3, order 1
SURFACE = [("long", 4, 5, 300, 3, 0), ("long-unequal", 3, 4, 300, 3, 0), ("fused", 6, 5, 16, 3, 1)]


@pytest.mark.parametrize("route,A,B,T,d,n", SURFACE)
@pytest.mark.parametrize("weighted", [False, True])
def test_compute_gram_grad_Y(gpu, route, A, B, T, d, n, weighted):
    import sigsvgd_amd.sigkernel as sk
    from sigsvgd_amd import ops

    TY = 180 if route == "long-unequal" else T
    assert ops.gram_takes(A, B, T, d, n) is (route == "fused")
    Xn, Yn, X, Y, rng = _leafs(gpu, A, B, T, TY, d, 20 + A)
    W = rng.uniform(0.5, 1.5, (A, B)) if weighted else None
    Kr, gXr, gYr = oracle_both_slots(Xn, Yn, 0.8, n, False, 0, W)
    kernel = sk.SigKernel(sk.RBFKernel(0.8), n)
    K = kernel.compute_Gram(X, Y, grad_Y=True)
    (K.sum() if W is None else (K * torch.as_tensor(W, device=gpu)).sum()).backward()
    tolK = 1e-9 if route != "fused" else 1e-5  # (the fused kernels' own bound: fp32 sweeps)
    assert rel_entry(np64(K), Kr, 0.0) < tolK
    assert rel_max(np64(X.grad), gXr) < 1e-5
    assert Y.grad is not None and Y.grad.shape == Y.shape and Y.grad.dtype == Y.dtype
    assert rel_max(np64(Y.grad), gYr) < 1e-5
    # the default: the first slot only
    X2, Y2 = X.detach().clone().requires_grad_(True), Y.detach().clone().requires_grad_(True)
    kernel.compute_Gram(X2, Y2).sum().backward()
    assert Y2.grad is None and rel_max(np64(X2.grad), oracle_both_slots(Xn, Yn, 0.8, n, False, 0, None)[1]) < 1e-5
    # Y alone
    Y3 = Y.detach().clone().requires_grad_(True)
    K3 = kernel.compute_Gram(X.detach(), Y3, grad_Y=True)
    (K3.sum() if W is None else (K3 * torch.as_tensor(W, device=gpu)).sum()).backward()
    assert rel_max(np64(Y3.grad), gYr) < 1e-5 and rel_entry(np64(K3), Kr, 0.0) < tolK


@pytest.mark.parametrize("route,A,T,d,n", [("long", 5, 300, 3, 0), ("fused", 6, 16, 3, 1)])
def test_one_tensor_in_both_slots(gpu, route, A, T, d, n):
    """grad_Y=True with one leaf in both slots: autograd adds the two slots, which is sym=True; with sym=True it raises."""
    import sigsvgd_amd.sigkernel as sk

    rng = np.random.default_rng(31)
    Xn = sized_walks(rng, A, T, d)
    kernel = sk.SigKernel(sk.RBFKernel(0.8), n)
    grads = []
    for kw in (dict(grad_Y=True), dict(sym=True)):
        X = torch.as_tensor(Xn, dtype=F64, device=gpu).requires_grad_(True)
        kernel.compute_Gram(X, X, **kw).sum().backward()
        grads.append(np64(X.grad))
    _, gr = c_oracle.gram_fwd_bwd(Xn, Xn, h=0.8, n=n, grad_out=np.full((A, A), 2.0))
    assert rel_max(grads[0], gr) < 1e-5 and rel_max(grads[1], gr) < 1e-5
    assert rel_max(grads[0], grads[1]) < 1e-5
    with pytest.raises(ValueError):
        kernel.compute_Gram(X, X, sym=True, grad_Y=True)


@pytest.mark.parametrize("route,A,B,T,d,n", [("long", 4, 5, 300, 3, 0), ("fused", 6, 5, 16, 3, 1)])
def test_compute_mmd_grad_Y(gpu, route, A, B, T, d, n):
    """Y.grad of compute_mmd(X, Y, grad_Y=True) = (1/B^2) [both slots of sum K_YY] - (2/(A B)) [second slot of sum K_XY];
    the default lacks the cross term."""
    import sigsvgd_amd.sigkernel as sk

    Xn, Yn, X, Y, _ = _leafs(gpu, A, B, T, T, d, 40)
    h = 0.8
    _, gyy = c_oracle.gram_fwd_bwd(Yn, Yn, h=h, n=n, grad_out=np.full((B, B), 2.0))
    _, _, gxy = oracle_both_slots(Xn, Yn, h, n, False, 0, None)
    ref = gyy / B**2 - 2.0 * gxy / (A * B)
    kernel = sk.SigKernel(sk.RBFKernel(h), n)
    kernel.compute_mmd(X, Y, grad_Y=True).backward()
    assert rel_max(np64(Y.grad), ref) < 1e-5
    Y2 = Y.detach().clone().requires_grad_(True)
    kernel.compute_mmd(X.detach(), Y2).backward()
    assert rel_max(np64(Y2.grad), gyy / B**2) < 1e-5  # (the default: the self term alone)


def test_user_static_kernel_grad_Y(gpu):
    """A user static kernel with grad_Y=True: Y stays in the graph and autograd gives it the same gradient as the built-in
    RBF's two-slot launch (the user-route tolerances of test_gpu_long.py: K 1e-9, gradients 1e-5)."""
    import sigsvgd_amd.sigkernel as sk

    _, _, X, Y, rng = _leafs(gpu, 4, 3, 300, 300, 3, 50)
    W = torch.as_tensor(rng.uniform(0.5, 1.5, (4, 3)), device=gpu)
    out = []
    for static in (sk.RBFKernel(0.8), DisguisedRBF(0.8)):
        Xl, Yl = X.detach().clone().requires_grad_(True), Y.detach().clone().requires_grad_(True)
        K = sk.SigKernel(static, 0).compute_Gram(Xl, Yl, grad_Y=True)
        (K * W).sum().backward()
        out.append((np64(K), np64(Xl.grad), np64(Yl.grad)))
    assert rel_entry(out[0][0], out[1][0], 0.0) < 1e-9
    assert rel_max(out[0][1], out[1][1]) < 1e-5 and rel_max(out[0][2], out[1][2]) < 1e-5
    Yd = Y.detach().clone().requires_grad_(True)
    sk.SigKernel(DisguisedRBF(0.8), 0).compute_Gram(X.detach().clone().requires_grad_(True), Yd).sum().backward()
    assert Yd.grad is None  # the default detaches Y, as before


def _count_calls(monkeypatch):
    from sigsvgd_amd import ops

    calls = []
    real = ops.gram_long_fwd_bwd2

    def counted(*a, **kw):
        calls.append(kw.get("y_is_x", a[8] if len(a) > 8 else False))
        return real(*a, **kw)

    monkeypatch.setattr(ops, "gram_long_fwd_bwd2", counted)
    return calls


def test_svgd_step_runs_the_y_is_x_launch(gpu, monkeypatch):
    """SVGD.step() with the signature kernel at the long-route shape of test_gpu_long.py's SVGD test: against the oracle's
    step and against the user route's, as that test checks it (1e-5 of the largest entry), through one Y-is-X launch."""
    import sigsvgd_amd.sigkernel as sk
    from oracle import sigkernel_oracle as O
    from sigsvgd_amd.inference import SVGD
    from sigsvgd_amd.kernels import SignatureKernel

    rng = np.random.default_rng(2)
    N, T, d, h, lr = 8, 300, 3, 2.0, 0.05
    Xn = sized_walks(rng, N, T, d)
    sn = rng.standard_normal((N, T, d))
    Kr, gr = c_oracle.gram_fwd_bwd(Xn, Xn, h=h, n=0)
    X_ref, v_ref, _ = O.svgd_step_manual(Xn, sn, Kr, gr, lr)
    X = torch.as_tensor(Xn, dtype=F64, device=gpu)
    score = torch.as_tensor(sn, dtype=F64, device=gpu)
    calls = _count_calls(monkeypatch)
    out = []
    for kernel in (SignatureKernel(lambda _: h, depth=0), sk.SigKernel(DisguisedRBF(h), 0)):
        Xnew, info = SVGD(kernel, optimizer_class=None, lr=lr).step(X.clone(), score)
        out.append((np64(Xnew), np64(info["grad"]).reshape(N, T, d)))
    assert calls == [True]  # (the user route launches the PDE on its grid, not this kernel)
    assert rel_max(out[0][0], X_ref) < 1e-5 and rel_max(out[0][1], v_ref) < 1e-5
    assert rel_max(out[0][0], out[1][0]) < 1e-5 and rel_max(out[0][1], out[1][1]) < 1e-5


def test_y_is_x_routing_of_the_surface(gpu, monkeypatch):
    """Where the long route runs with Y = X -- the same tensor in both slots, gram_and_grad(X), equal values found by the
    value check -- the launch is the Y-is-X one wherever `_long_yx_route` says so (gradient launches
    of single-pair items, forward-only launches of many pairs); a distinct Y takes the ordered launch."""
    import sigsvgd_amd.sigkernel as sk

    cus = device_cus()
    route = lambda A, want_grad: sk._long_yx_route(True, A, want_grad, cus)
    assert route(8, True) and route(32, True) and not route(8, False) and not sk._long_yx_route(False, 8, True, cus)
    rng = np.random.default_rng(7)
    X = torch.as_tensor(sized_walks(rng, 6, 300, 2), dtype=F64, device=gpu)
    Y = torch.as_tensor(sized_walks(rng, 6, 300, 2), dtype=F64, device=gpu)
    kernel = sk.SigKernel(sk.RBFKernel(1.0), 0)
    calls = _count_calls(monkeypatch)
    K0 = kernel.compute_Gram(X, X)  # forward only, few pairs: the ordered launch
    assert calls == []
    Xg = X.clone().requires_grad_(True)
    K1 = kernel.compute_Gram(Xg, Xg)
    K1.sum().backward()
    K2, g2 = kernel.gram_and_grad(X)
    assert calls == [True, True]
    iu = torch.triu_indices(6, 6, device=gpu)
    assert torch.equal(K1.detach(), K2) and torch.equal(K2, K2.T) and torch.equal(K0[iu[0], iu[1]], K2[iu[0], iu[1]])
    assert rel_max(np64(Xg.grad), np64(g2)) < 1e-12
    kernel.compute_Gram(X, Y)
    kernel.gram_and_grad(X, Y)
    assert calls == [True, True]
    big = torch.as_tensor(sized_walks(rng, 32, 300, 2), dtype=F64, device=gpu)  # (the value check starts at 32 paths)
    kernel.compute_Gram(big.clone().requires_grad_(True), big.clone())
    assert calls == [True, True, True]
    # past single-pair items the gradient launch stays ordered; many pairs send the forward-only launch through Y-is-X
    A = 64
    assert not route(A, True) and route(A, False), cus
    wide = torch.as_tensor(sized_walks(rng, A, 300, 2), dtype=F64, device=gpu)
    Kg, _ = kernel.gram_and_grad(wide)
    assert calls == [True, True, True]
    Kw = kernel.compute_Gram(wide, wide)
    assert calls == [True, True, True, True]
    iu = torch.triu_indices(A, A, device=gpu)
    assert torch.equal(Kw, Kw.T) and torch.equal(Kw[iu[0], iu[1]], Kg[iu[0], iu[1]])
