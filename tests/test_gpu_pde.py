"""The signature PDE on a caller's static-kernel grid (csrc/sig_pde.hip, `ops.pde_*`, `ops.PDESolve`) and the user
static-kernel route of `sigsvgd_amd.sigkernel` against the fp64 oracle and against the built-in kernels."""
import numpy as np
import pytest
import torch

from oracle import sigkernel_oracle as O
from parity import DisguisedRBF, gram_and_xgrad, rel_entry, rel_max
from plans import device_cus, pde_plan

pytestmark = pytest.mark.gpu


def ref_pde(G, n, naive=False, grad_out=None):
    """(K [npairs], dG [npairs, M, N]) of the oracle's pieces for grids G [npairs, M, N] (gram_backward's convention)."""
    G = np.asarray(G, dtype=np.float64)
    npairs, M, N = G.shape
    g = O.refine(O.increments(G), n)
    Kf = O.pde_sweep(g, naive)
    GG = O.gg_matrix(Kf, g, naive)
    r = 2**n
    S = GG.reshape(npairs, M - 1, r, N - 1, r).sum(axis=(2, 4)) / float(r * r)
    R = np.zeros((npairs, M, N))
    R[:, 1:, 1:] += S
    R[:, :-1, :-1] += S
    R[:, 1:, :-1] -= S
    R[:, :-1, 1:] -= S
    w = np.ones(npairs) if grad_out is None else np.asarray(grad_out, dtype=np.float64)
    return Kf[:, -1, -1], R * w[:, None, None]


def grid_walks(rng, B, T, d, step=0.15):
    return np.cumsum(step * rng.standard_normal((B, T, d)), axis=1)


def grids(rng, M, N, d=2, h=1.0, A=2, B=2):
    X, Y = grid_walks(rng, A, M, d), grid_walks(rng, B, N, d)
    return O.static_gram(X, Y, O.RBF, h).reshape(A * B, M, N)


@pytest.mark.parametrize("naive", [False, True])
@pytest.mark.parametrize("n", [0, 1, 2, 4])
@pytest.mark.parametrize("M,N", [(2, 2), (3, 5), (10, 10), (17, 33), (64, 64), (65, 40)])
def test_primitive_matches_oracle(gpu, M, N, n, naive):
    from sigsvgd_amd import ops

    rng = np.random.default_rng(M * 1000 + N * 10 + n)
    G = grids(rng, M, N)
    go = rng.uniform(0.5, 1.5, G.shape[0])
    Kr, dGr = ref_pde(G, n, naive, go)
    Gt = torch.as_tensor(G, device=gpu)
    K = ops.pde_fwd(Gt, n, naive).cpu().numpy()
    assert rel_entry(K, Kr, 0.1) < 1e-9
    K2, dG = ops.pde_fwd_bwd(Gt, n, torch.as_tensor(go, device=gpu), naive)
    assert rel_entry(K2.cpu().numpy(), Kr, 0.1) < 1e-9
    assert rel_max(dG.cpu().numpy(), dGr) < 1e-5
    # fp32 grids: K of the same rounded grid, in fp32
    G32 = G.astype(np.float32)
    Kr32, dGr32 = ref_pde(G32, n, naive)
    K32, dG32 = ops.pde_fwd_bwd(torch.as_tensor(G32, device=gpu), n, None, naive)
    assert K32.dtype == torch.float32 and dG32.dtype == torch.float32
    assert rel_entry(K32.cpu().double().numpy(), Kr32, 0.1) < 1e-5
    assert rel_max(dG32.cpu().double().numpy(), dGr32) < 1e-5


@pytest.mark.parametrize("naive", [False, True])
@pytest.mark.parametrize("M,N,n,d,pick", [(257, 257, 0, 2, None), (100, 100, 3, 3, [0, 7, 35]), (40, 300, 1, 2, None)])
def test_long_grids(gpu, M, N, n, d, pick, naive):
    """Grids past the built-in kernels' LDS limit (T = 256 at order 0 is UNSUPPORTED there), the reference's arm-script
    shape ([6, 100, 3] at order 3: P = 792) and a refined ring that wraps (N - 1 = 299 columns at order 1)."""
    from sigsvgd_amd import ops

    rng = np.random.default_rng(M + N + n)
    if pick is None:
        G = grids(rng, M, N, d, h=2.0, A=1, B=2)
    else:
        X = grid_walks(rng, 6, M, d, 0.05)
        G = O.static_gram(X, X, O.RBF, 1.0).reshape(36, M, N)
    K, dG = ops.pde_fwd_bwd(torch.as_tensor(G, device=gpu), n, None, naive)
    sel = list(range(G.shape[0])) if pick is None else pick
    Kr, dGr = ref_pde(G[sel], n, naive)
    assert rel_entry(K.cpu().numpy()[sel], Kr, 0.1) < 1e-9
    assert rel_max(dG.cpu().numpy()[sel], dGr) < 1e-5


@pytest.mark.parametrize("sym", [False, True])
@pytest.mark.parametrize("n", [0, 2])
def test_disguised_rbf_matches_builtin(gpu, n, sym):
    import sigsvgd_amd.sigkernel as sk

    rng = np.random.default_rng(7 + n)
    sigma, A = 0.8, 6
    X = torch.as_tensor(grid_walks(rng, A, 12, 3), device=gpu)
    Y = torch.as_tensor(grid_walks(rng, A, 12, 3), device=gpu)
    W = torch.as_tensor(rng.uniform(0.5, 1.5, (A, A)), device=gpu)
    Ku, gu = gram_and_xgrad(sk.SigKernel(DisguisedRBF(sigma), n), X, Y, W, sym)
    Kb, gb = gram_and_xgrad(sk.SigKernel(sk.RBFKernel(sigma), n), X, Y, W, sym)
    Wn = W.cpu().numpy()
    Yn = X.cpu().numpy() if sym else Y.cpu().numpy()
    Kr, gr = O.gram_backward(X.cpu().numpy(), Yn, Wn, O.RBF, sigma, n, sym=sym)
    assert Ku.dtype == torch.float64
    assert rel_entry(Ku.cpu().numpy(), Kr, 0.1) < 1e-5 and rel_entry(Ku.cpu().numpy(), Kb.cpu().numpy(), 0.1) < 1e-5
    assert rel_max(gu.cpu().numpy(), gr) < 1e-5 and rel_max(gu.cpu().numpy(), gb.cpu().numpy()) < 1e-5
    # gram_and_grad (what SVGD calls) gives the same
    Kg, gg = sk.SigKernel(DisguisedRBF(sigma), n).gram_and_grad(X, None if sym else Y, W, sym=sym)
    assert rel_entry(Kg.cpu().numpy(), Kr, 0.1) < 1e-5 and rel_max(gg.cpu().numpy(), gr) < 1e-5


def test_disguised_rbf_unequal_lengths(gpu):
    import sigsvgd_amd.sigkernel as sk

    rng = np.random.default_rng(3)
    X = torch.as_tensor(grid_walks(rng, 4, 9, 2), device=gpu)
    Y = torch.as_tensor(grid_walks(rng, 5, 14, 2), device=gpu)
    W = torch.ones(4, 5, dtype=torch.float64, device=gpu)
    Ku, gu = gram_and_xgrad(sk.SigKernel(DisguisedRBF(1.0), 1), X, Y, W, False)
    Kb, gb = gram_and_xgrad(sk.SigKernel(sk.RBFKernel(1.0), 1), X, Y, W, False)
    assert Ku.shape == (4, 5) and gu.shape == X.shape
    assert rel_entry(Ku.cpu().numpy(), Kb.cpu().numpy(), 0.1) < 1e-5 and rel_max(gu.cpu().numpy(), gb.cpu().numpy()) < 1e-5


class ARDRBF(torch.nn.Module):
    """exp(-sum_c (x_c - y_c)^2 / l_c) with a learnable lengthscale per channel."""

    def __init__(self, ls):
        super().__init__()
        self.ls = torch.nn.Parameter(ls)

    def Gram_matrix(self, X, Y):
        Xs, Ys = X / self.ls.sqrt(), Y / self.ls.sqrt()
        dist = (Xs**2).sum(-1)[:, None, :, None] + (Ys**2).sum(-1)[None, :, None, :] - 2.0 * torch.einsum("ipk,jqk->ijpq", Xs, Ys)
        return torch.exp(-dist)


class Poly:
    def Gram_matrix(self, X, Y):
        return (1.0 + 0.5 * torch.einsum("ipk,jqk->ijpq", X, Y)) ** 2


def _oracle_chain(static, X, Y, W, n, naive, params=()):
    """K and the gradients of sum(W * K) w.r.t. X and `params` on the CPU: fp64 oracle PDE, torch autograd for the chain."""
    Xc = X.detach().cpu().requires_grad_(True)
    G = static.Gram_matrix(Xc, Y.detach().cpu())
    A, B, M, N = G.shape
    Kr, dGr = ref_pde(G.detach().numpy().reshape(A * B, M, N), n, naive, W.cpu().numpy().reshape(-1))
    grads = torch.autograd.grad(G, (Xc,) + tuple(params), torch.as_tensor(dGr.reshape(A, B, M, N)))
    return Kr.reshape(A, B), [g.numpy() for g in grads]


@pytest.mark.parametrize("naive", [False, True])
def test_ard_and_polynomial_kernels(gpu, naive):
    import sigsvgd_amd.sigkernel as sk

    rng = np.random.default_rng(11)
    n = 2
    X = torch.as_tensor(grid_walks(rng, 4, 8, 3), device=gpu)
    Y = torch.as_tensor(grid_walks(rng, 3, 11, 3), device=gpu)
    W = torch.as_tensor(rng.uniform(0.5, 1.5, (4, 3)), device=gpu)
    ls0 = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)
    ard = ARDRBF(ls0.clone()).to(gpu)
    Xg = X.clone().requires_grad_(True)
    K = sk.SigKernel(ard, n, _naive_solver=naive).compute_Gram(Xg, Y)
    gX, gls = torch.autograd.grad((K * W).sum(), (Xg, ard.ls))
    ard_cpu = ARDRBF(ls0.clone())
    Kr, (gXr, glsr) = _oracle_chain(ard_cpu, X, Y, W, n, naive, (ard_cpu.ls,))
    assert rel_entry(K.detach().cpu().numpy(), Kr, 0.1) < 1e-5
    assert rel_max(gX.cpu().numpy(), gXr) < 1e-5 and rel_max(gls.cpu().numpy(), glsr) < 1e-5
    Xg = X.clone().requires_grad_(True)
    K = sk.SigKernel(Poly(), 1, _naive_solver=naive).compute_Gram(Xg, Y)
    (gX,) = torch.autograd.grad((K * W).sum(), Xg)
    Kr, (gXr,) = _oracle_chain(Poly(), X, Y, W, 1, naive)
    assert rel_entry(K.detach().cpu().numpy(), Kr, 0.1) < 1e-5 and rel_max(gX.cpu().numpy(), gXr) < 1e-5


def test_gradcheck_naive(gpu):
    """With the naive stencil the GG convention is the exact adjoint: torch's finite differences agree."""
    import sigsvgd_amd.sigkernel as sk

    rng = np.random.default_rng(5)
    X = torch.as_tensor(grid_walks(rng, 2, 3, 2, 0.3), device=gpu).requires_grad_(True)
    Y = torch.as_tensor(grid_walks(rng, 2, 4, 2, 0.3), device=gpu)
    ls = torch.tensor([0.7, 1.3], dtype=torch.float64, device=gpu, requires_grad=True)

    class Fn(torch.nn.Module):
        def Gram_matrix(self, A, B):
            return ARDRBF.Gram_matrix(self, A, B)

    def f(Xv, lsv):
        k = Fn()
        k.ls = lsv
        return sk.SigKernel(k, 1, _naive_solver=True).compute_Gram(Xv, Y)

    assert torch.autograd.gradcheck(f, (X, ls), eps=1e-6, atol=1e-6, rtol=1e-4)


def test_compute_kernel_distance_mmd(gpu):
    import sigsvgd_amd.sigkernel as sk

    rng = np.random.default_rng(9)
    n, sigma = 1, 1.2
    X = torch.as_tensor(grid_walks(rng, 5, 10, 2), device=gpu)
    Y = torch.as_tensor(grid_walks(rng, 5, 10, 2), device=gpu)
    k = sk.SigKernel(DisguisedRBF(sigma), n)
    kb = k.compute_kernel(X, Y)
    assert kb.shape == (5,)
    assert rel_entry(kb.cpu().numpy(), k.compute_Gram(X, Y).diagonal().cpu().numpy(), 0.1) < 1e-12
    Xn, Yn = X.cpu().numpy(), Y.cpu().numpy()
    Kxx, Kyy, Kxy = (O.gram(a, b, O.RBF, sigma, n) for (a, b) in [(Xn, Xn), (Yn, Yn), (Xn, Yn)])
    dist = np.diag(Kxx).mean() + np.diag(Kyy).mean() - 2 * np.diag(Kxy).mean()
    mmd = Kxx.mean() + Kyy.mean() - 2 * Kxy.mean()
    assert abs(float(k.compute_distance(X, Y)) - dist) < 1e-9 * max(1.0, abs(dist))
    assert abs(float(k.compute_mmd(X, Y)) - mmd) < 1e-9 * max(1.0, abs(mmd))


def test_svgd_step_with_user_kernel(gpu):
    import sigsvgd_amd.sigkernel as sk
    from sigsvgd_amd.inference import SVGD

    rng = np.random.default_rng(2)
    X = torch.as_tensor(grid_walks(rng, 16, 10, 2), dtype=torch.float32, device=gpu)
    score = torch.as_tensor(rng.standard_normal((16, 10, 2)), dtype=torch.float32, device=gpu)
    out = []
    for static in (DisguisedRBF(1.0), sk.RBFKernel(1.0)):
        s = SVGD(sk.SigKernel(static, 2), optimizer_class=None, lr=0.05)
        Xn, info = s.step(X.clone(), score)
        out.append((Xn.detach().cpu().numpy(), info["grad"].cpu().numpy()))
    assert rel_max(out[0][0], out[1][0]) < 1e-5 and rel_max(out[0][1], out[1][1]) < 1e-5


def test_pde_determinism(gpu):
    from sigsvgd_amd import ops

    rng = np.random.default_rng(1)
    for (M, N, n) in [(10, 10, 4), (200, 150, 0), (33, 17, 2)]:
        G = torch.as_tensor(grids(rng, M, N, A=8, B=8), device=gpu)
        go = torch.as_tensor(rng.standard_normal(G.shape[0]), device=gpu)
        K1, d1 = ops.pde_fwd_bwd(G, n, go)
        K2, d2 = ops.pde_fwd_bwd(G, n, go)
        assert torch.equal(K1, K2) and torch.equal(d1, d2)


# ---- the plan's branches (tests/plans.pde_plan mirrors pde_make_plan; test_pde_cabi.py pins it to the library) --------
PDE_BRANCHES = [
    # the increment ring exactly full, then wrapping once, at orders 0, 1, 2 (Wcap = 128, 256, 512 columns)
    (70, 129, 0, "full"), (70, 130, 0, "wrap"), (40, 257, 1, "full"), (40, 258, 1, "wrap"), (20, 513, 2, "full"),
    (20, 514, 2, "wrap"),
    # orders 7 to 10 (nrow = 1: a band of 64 rows is part of one coarse row)
    (9, 9, 7, "nrow1"), (9, 9, 8, "nrow1"), (3, 9, 10, "nrow1"), (9, 3, 10, "nrow1"),
    # a last band of one row; a single coarse column or row against a long grid
    (66, 40, 0, "L1"), (258, 20, 0, "L1"), (300, 2, 0, "Q1"), (2, 300, 0, "P1"),
]


@pytest.mark.parametrize("naive", [False, True])
@pytest.mark.parametrize("M,N,n,regime", PDE_BRANCHES)
def test_plan_branches_match_oracle(gpu, M, N, n, regime, naive):
    from sigsvgd_amd import ops

    pl = pde_plan(4, M, N, n, True, device_cus())
    assert pl is not None and {"full": N - 1 == pl["W"], "wrap": N - 1 == pl["W"] + 1,
                               "nrow1": pl["nrow"] == 1 and pl["P"] > 64, "L1": pl["P"] % 64 == 1 and pl["P"] > 64,
                               "Q1": pl["Q"] == 1, "P1": pl["P"] == 1}[regime], pl
    rng = np.random.default_rng(M * 1000 + N * 10 + n)
    G = grids(rng, M, N, h=2.0)
    go = rng.uniform(0.5, 1.5, G.shape[0])
    Kr, dGr = ref_pde(G, n, naive, go)
    Gt = torch.as_tensor(G, device=gpu)
    K, dG = ops.pde_fwd_bwd(Gt, n, torch.as_tensor(go, device=gpu), naive)
    assert rel_entry(K.cpu().numpy(), Kr, 0.1) < 1e-9
    assert rel_max(dG.cpu().numpy(), dGr) < 1e-5
    assert torch.equal(ops.pde_fwd(Gt, n, naive), K)


@pytest.mark.parametrize("naive", [False, True])
def test_more_pairs_than_resident_waves(gpu, naive):
    """2500 grids of 10 x 10: more pairs than the launch's waves, so each wave solves several pairs in turn."""
    from sigsvgd_amd import ops

    pl = pde_plan(2500, 10, 10, 0, True, device_cus())
    assert pl["grid"] < 2500, pl
    rng = np.random.default_rng(2500 + naive)
    G = grids(rng, 10, 10, d=3, A=50, B=50)
    go = rng.uniform(0.5, 1.5, G.shape[0])
    Kr, dGr = ref_pde(G, 0, naive, go)
    K, dG = ops.pde_fwd_bwd(torch.as_tensor(G, device=gpu), 0, torch.as_tensor(go, device=gpu), naive)
    assert rel_entry(K.cpu().numpy(), Kr, 0.1) < 1e-9
    assert rel_max(dG.cpu().numpy(), dGr) < 1e-5
