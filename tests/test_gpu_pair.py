"""Paired signature kernels (the paired mode of csrc/gram_long.hip, `ops.pair_*`, `SigKernel.compute_kernel` and
`compute_distance`): K against the C oracle and bit for bit against the Gram long route, both gradients against the oracle
(the second slot through the identity d2 k(X, Y) = d1 k(Y, X)), the autograd surface, reproducibility and refusal."""
import numpy as np
import pytest
import torch

from oracle import c_oracle
from oracle import sigkernel_oracle as O
from parity import DisguisedRBF, np64, rel_entry, rel_max, sized_walks

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32


def c_pair_first_slot(X, Y, h, n, naive, kind, w):
    """C oracle per pair: (K [A], d(w_i k(X_i, Y_i))/dX_i [A, TX, d]), the shorter path of a pair padded with its last point
    (exact) and the gradient of a padded X folded back onto its points."""
    from sigsvgd_amd import ops

    A, TX = X.shape[:2]
    T = max(TX, Y.shape[1])
    pad = lambda P: ops.pad_to_length(torch.as_tensor(P), T).numpy()
    Xp, Yp = pad(X), pad(Y)
    K, g = np.empty(A), np.empty((A, T, X.shape[2]))
    nthreads = 2 if (T - 1) << n > 4096 else 0
    for i in range(A):
        Ki, gi = c_oracle.gram_fwd_bwd(Xp[i:i + 1], Yp[i:i + 1], h=h, n=n, naive=naive, kind=kind, grad_out=w[i:i + 1, None],
                                       nthreads=nthreads)
        K[i], g[i] = Ki[0, 0], gi[0]
    return K, ops.fold_padded_grad(torch.as_tensor(g), TX).numpy()


# (A, TX, TY, d, n, kind, naive, io)
CASES = [
    (6, 10, 10, 2, 4, 0, False, F64),      # notebook
    (16, 64, 64, 7, 0, 0, False, F64),     # SVGD's C4 batch
    (16, 64, 64, 7, 0, 0, False, F32),
    (3, 100, 100, 3, 3, 0, False, F64),    # arm-spline example
    (3, 40, 70, 2, 0, 0, False, F64),      # TX != TY
    (3, 70, 40, 2, 1, 0, False, F64),
    (2, 1024, 1024, 2, 0, 0, False, F64),  # long
    (2, 300, 300, 17, 0, 0, False, F64),   # channels past the 16 kept in registers
    (2, 300, 300, 33, 0, 0, False, F64),
    (3, 60, 60, 3, 1, 1, False, F64),      # linear kernel
    (3, 60, 50, 3, 1, 1, True, F64),
    (3, 50, 50, 2, 2, 0, True, F64),       # naive solver
    (2, 129, 129, 2, 0, 0, False, F64),    # ring exactly full
    (2, 130, 130, 2, 0, 1, True, F64),     # ring wrapping once
    (2, 258, 257, 2, 1, 0, False, F64),
    (2, 66, 66, 2, 0, 0, False, F64),      # a last band of one row
    (2, 258, 258, 3, 0, 1, True, F64),
    (2, 9, 9, 2, 8, 0, False, F64),        # nrow = 1
]


def _case_id(c):
    A, TX, TY, d, n, kind, naive, io = c
    return f"A{A}-T{TX}x{TY}-d{d}-n{n}-{'lin' if kind else 'rbf'}{'-naive' if naive else ''}-{'f32' if io == F32 else 'f64'}"


@pytest.mark.parametrize("A,TX,TY,d,n,kind,naive,io", CASES, ids=[_case_id(c) for c in CASES])
def test_pairs_match_oracle_and_gram_long(gpu, A, TX, TY, d, n, kind, naive, io):
    from sigsvgd_amd import ops

    rng = np.random.default_rng(A * 1000 + TX * 7 + TY + 31 * d + n + 5 * kind + naive)
    h = 0.5
    X, Y = sized_walks(rng, A, TX, d, d**-0.5), sized_walks(rng, A, TY, d, d**-0.5)
    w = rng.uniform(-1.5, 1.5, A)
    Xt, Yt = torch.as_tensor(X, dtype=io, device=gpu), torch.as_tensor(Y, dtype=io, device=gpu)
    wt = torch.as_tensor(w, device=gpu)
    K, gX, gY = ops.pair_fwd_bwd(Xt, Yt, 1.0 / h, n, kind, wt, naive)
    assert K.shape == (A,) and gX.shape == Xt.shape and gY.shape == Yt.shape
    assert K.dtype == gX.dtype == gY.dtype == io
    Kr, gXr = c_pair_first_slot(X, Y, h, n, naive, kind, w)
    _, gYr = c_pair_first_slot(Y, X, h, n, naive, kind, w)  # the second slot is the first slot of the swapped pair
    assert rel_entry(np64(K), Kr, 0.0) < (1e-9 if io == F64 else 2.0**-23)
    assert rel_max(np64(gX), gXr) < 1e-5
    assert rel_max(np64(gY), gYr) < 1e-5
    # the forward alone, and each gradient alone, give the same bits
    K0 = ops.pair_fwd(Xt, Yt, 1.0 / h, n, kind, naive)
    assert torch.equal(K0, K)
    Kx, gx, none_y = ops.pair_fwd_bwd(Xt, Yt, 1.0 / h, n, kind, wt, naive, want_y=False)
    Ky, none_x, gy = ops.pair_fwd_bwd(Xt, Yt, 1.0 / h, n, kind, wt, naive, want_x=False)
    assert none_x is None and none_y is None
    assert torch.equal(Kx, K) and torch.equal(Ky, K) and torch.equal(gx, gX) and torch.equal(gy, gY)
    # the Gram long route shares the arithmetic: K is its diagonal bit for bit, gY its first slot on the swapped pairs
    KL = ops.gram_long_fwd(Xt, Yt, 1.0 / h, n, kind, naive)
    assert torch.equal(KL.diagonal(), K)
    _, gYL = ops.gram_long_fwd_bwd(Yt, Xt, 1.0 / h, n, kind, torch.diag(wt), naive)
    assert rel_max(np64(gY), np64(gYL)) < 1e-5


def test_same_buffer_in_both_slots(gpu):
    from sigsvgd_amd import ops

    rng = np.random.default_rng(12)
    X = torch.as_tensor(sized_walks(rng, 5, 30, 3), dtype=F64, device=gpu)
    K, gX, gY = ops.pair_fwd_bwd(X, X, 2.0, 1)
    K2, gX2, gY2 = ops.pair_fwd_bwd(X, X.clone(), 2.0, 1)
    assert torch.equal(K, K2) and torch.equal(gX, gX2) and torch.equal(gY, gY2)


# ---- the autograd surface -----------------------------------------------------------------------------------------------
def _np_first_slot(X, Y, h, n, naive=False, w=None, kind=O.RBF):
    """numpy oracle per pair: (K [A], d(w_i k(X_i, Y_i))/dX_i)"""
    A = X.shape[0]
    w = np.ones(A) if w is None else w
    K, g = np.empty(A), np.empty_like(X, dtype=np.float64)
    for i in range(A):
        Ki, gi = O.gram_backward(X[i:i + 1], Y[i:i + 1], w[i:i + 1, None], kind, h, n, naive)
        K[i], g[i] = Ki[0, 0], gi[0]
    return K, g


def _inputs(gpu, A=6, TX=12, TY=9, d=3, seed=21, io=F64):
    rng = np.random.default_rng(seed)
    X = np.cumsum(0.2 * rng.standard_normal((A, TX, d)), 1)
    Y = np.cumsum(0.2 * rng.standard_normal((A, TY, d)), 1)
    return X, Y, torch.as_tensor(X, dtype=io, device=gpu), torch.as_tensor(Y, dtype=io, device=gpu)


def test_compute_kernel_gradients_of_both_slots(gpu):
    import sigsvgd_amd.sigkernel as sk

    X, Y, Xt, Yt = _inputs(gpu)
    sigma, n = 0.8, 2
    w = np.random.default_rng(1).uniform(-1, 2, X.shape[0])
    Xg, Yg = Xt.clone().requires_grad_(True), Yt.clone().requires_grad_(True)
    K = sk.SigKernel(sk.RBFKernel(sigma), n).compute_kernel(Xg, Yg)
    (K * torch.as_tensor(w, device=gpu)).sum().backward()
    Kr, gXr = _np_first_slot(X, Y, sigma, n, w=w)
    _, gYr = _np_first_slot(Y, X, sigma, n, w=w)
    assert rel_entry(np64(K), Kr, 0.0) < 1e-9
    assert Yg.grad is not None  # (the Gram diagonal gave None)
    assert rel_max(np64(Xg.grad), gXr) < 1e-5 and rel_max(np64(Yg.grad), gYr) < 1e-5


@pytest.mark.parametrize("naive", [False, True])
def test_compute_kernel_same_tensor_is_twice_the_first_slot(gpu, naive):
    import sigsvgd_amd.sigkernel as sk

    X, _, Xt, _ = _inputs(gpu, A=4, TX=8, d=2, seed=22)
    sigma, n = 1.1, 1
    k = sk.SigKernel(sk.RBFKernel(sigma), n, _naive_solver=naive)
    Xg = Xt.clone().requires_grad_(True)
    k.compute_kernel(Xg, Xg).sum().backward()
    _, g1 = _np_first_slot(X, X, sigma, n, naive)
    assert rel_max(np64(Xg.grad), 2.0 * g1) < 1e-5  # (the Gram diagonal gave 1x)
    if naive:  # the GG adjoint is exact for the naive stencil: central differences of sum_i k(X_i, X_i)
        f = lambda Z: float(k.compute_kernel(Z, Z).sum())
        rng = np.random.default_rng(3)
        for _ in range(4):
            i, t, c = int(rng.integers(4)), int(rng.integers(8)), int(rng.integers(2))
            e = torch.zeros_like(Xt)
            e[i, t, c] = 1e-6
            fd = (f(Xt + e) - f(Xt - e)) / 2e-6
            assert abs(fd - float(Xg.grad[i, t, c])) < 1e-6 * max(1.0, abs(fd))


def test_compute_distance_gradients(gpu):
    import sigsvgd_amd.sigkernel as sk

    X, Y, Xt, Yt = _inputs(gpu, A=5, TX=10, TY=10, d=2, seed=23)
    sigma, n = 0.9, 1
    A = X.shape[0]
    Xg, Yg = Xt.clone().requires_grad_(True), Yt.clone().requires_grad_(True)
    dist = sk.SigKernel(sk.RBFKernel(sigma), n).compute_distance(Xg, Yg)
    dist.backward()
    Kxx, gxx = _np_first_slot(X, X, sigma, n)
    Kyy, gyy = _np_first_slot(Y, Y, sigma, n)
    Kxy, gxy = _np_first_slot(X, Y, sigma, n)
    _, gyx = _np_first_slot(Y, X, sigma, n)
    assert abs(float(dist.detach()) - (Kxx.mean() + Kyy.mean() - 2 * Kxy.mean())) < 1e-9
    assert rel_max(np64(Xg.grad), (2.0 / A) * gxx - (2.0 / A) * gxy) < 1e-5
    assert rel_max(np64(Yg.grad), (2.0 / A) * gyy - (2.0 / A) * gyx) < 1e-5


def test_builtin_and_user_routes_agree(gpu):
    import sigsvgd_amd.sigkernel as sk

    _, _, Xt, Yt = _inputs(gpu, A=6, TX=20, TY=20, d=3, seed=24)
    out = []
    for static in (sk.RBFKernel(0.7), DisguisedRBF(0.7)):
        Xg, Yg = Xt.clone().requires_grad_(True), Yt.clone().requires_grad_(True)
        K = sk.SigKernel(static, 1).compute_kernel(Xg, Yg)
        (K * torch.linspace(-1, 2, 6, device=gpu, dtype=F64)).sum().backward()
        out.append((np64(K), np64(Xg.grad), np64(Yg.grad)))
    (Kb, gXb, gYb), (Ku, gXu, gYu) = out
    assert rel_entry(Kb, Ku, 0.0) < 1e-9
    assert rel_max(gXb, gXu) < 1e-5 and rel_max(gYb, gYu) < 1e-5


def test_gradcheck_naive_both_inputs(gpu):
    import sigsvgd_amd.sigkernel as sk

    rng = np.random.default_rng(5)
    X = torch.as_tensor(sized_walks(rng, 2, 3, 2, 0.3), dtype=F64, device=gpu).requires_grad_(True)
    Y = torch.as_tensor(sized_walks(rng, 2, 4, 2, 0.3), dtype=F64, device=gpu).requires_grad_(True)
    k = sk.SigKernel(sk.RBFKernel(0.5), 1, _naive_solver=True)
    assert torch.autograd.gradcheck(lambda a, b: k.compute_kernel(a, b), (X, Y), eps=1e-6, atol=1e-6, rtol=1e-4)


# ---- reproducibility, solve count, refusal --------------------------------------------------------------------------------
def test_pair_determinism(gpu):
    from sigsvgd_amd import ops

    rng = np.random.default_rng(7)
    for (A, TX, TY, n) in [(300, 64, 64, 0), (4, 300, 200, 0), (5, 20, 30, 3)]:
        X = torch.as_tensor(sized_walks(rng, A, TX, 3), device=gpu)
        Y = torch.as_tensor(sized_walks(rng, A, TY, 3), device=gpu)
        go = torch.as_tensor(rng.standard_normal(A), device=gpu)
        a = ops.pair_fwd_bwd(X, Y, 1.0, n, 0, go)
        b = ops.pair_fwd_bwd(X, Y, 1.0, n, 0, go)
        assert all(torch.equal(u, v) for u, v in zip(a, b))


def test_large_batch_stays_on_pairs(gpu, monkeypatch):
    """A = 512 paths of T = 64 with a gradient: no Gram launch at all (it would be 512^2 solves)."""
    import sigsvgd_amd.sigkernel as sk
    from sigsvgd_amd import ops

    def refuse(*a, **k):
        raise AssertionError("Gram launch from compute_kernel")

    for name in ("gram_fwd", "gram_fwd_bwd", "gram_long_fwd", "gram_long_fwd_bwd", "gram_sym_partial"):
        monkeypatch.setattr(ops, name, refuse)
    rng = np.random.default_rng(8)
    X = torch.as_tensor(sized_walks(rng, 512, 64, 7), device=gpu).requires_grad_(True)
    Y = torch.as_tensor(sized_walks(rng, 512, 64, 7), device=gpu).requires_grad_(True)
    k = sk.SigKernel(sk.RBFKernel(1.0), 0)
    K = k.compute_kernel(X, Y)
    K.sum().backward()
    assert K.shape == (512,) and X.grad is not None and Y.grad is not None
    assert bool(torch.isfinite(X.grad).all()) and bool(torch.isfinite(Y.grad).all())
    k.compute_distance(X.detach(), Y.detach())


def test_refuses_past_8192(gpu):
    import sigsvgd_amd.sigkernel as sk
    from sigsvgd_amd import ops

    X = torch.zeros(1, 8194, 2, device=gpu)
    with pytest.raises(RuntimeError, match="8192"):
        ops.pair_fwd(X, X, 1.0, 0)
    with pytest.raises(RuntimeError, match="8192"):
        ops.pair_fwd_bwd(X, X, 1.0, 0)
    with pytest.raises(RuntimeError, match="8192"):  # (no route takes it: the Gram diagonal refuses as well)
        sk.SigKernel(sk.RBFKernel(1.0), 0).compute_kernel(X, X)
