"""Long paths with the built-in static kernels (csrc/gram_long.hip, `ops.gram_long_*`, the routing of
`sigsvgd_amd.sigkernel`): against the C oracle, against the coverage kernel where both run, and against the user
static-kernel route (`DisguisedRBF`: the same RBF behind upstream's interface, solved by csrc/sig_pde.hip on the grid torch
builds).  Every RBF shape here except the overlap cases is one the fused Gram kernels refuse for LDS."""
import numpy as np
import pytest
import torch

from oracle import c_oracle

pytestmark = pytest.mark.gpu


def paths(rng, B, T, d, scale=1.0):
    """random walks of about `scale` overall size whatever their length"""
    return np.cumsum(scale / np.sqrt(T) * rng.standard_normal((B, T, d)), axis=1).astype(np.float32)


def relK(K, Kr):  # plain relative error per entry
    return float((np.abs(np.asarray(K, np.float64) - Kr) / np.abs(Kr)).max())


def relmax(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def np64(t):
    return t.detach().double().cpu().numpy()


class DisguisedRBF:
    """exp(-|x - y|^2 / sigma) behind upstream's interface only: the library cannot recognise it (user route)."""

    def __init__(self, sigma):
        self.sigma = sigma

    def Gram_matrix(self, X, Y):
        dist = (X**2).sum(-1)[:, None, :, None] + (Y**2).sum(-1)[None, :, None, :] - 2.0 * torch.einsum("ipk,jqk->ijpq", X, Y)
        return torch.exp(-dist / self.sigma)

    def batch_kernel(self, X, Y):
        dist = (X**2).sum(-1)[:, :, None] + (Y**2).sum(-1)[:, None, :] - 2.0 * torch.bmm(X, Y.transpose(1, 2))
        return torch.exp(-dist / self.sigma)


# (A, B, T, d, n, kind, naive, io, weights): weights "ones" / "rand" (non-uniform grad_out) / "sym" (sym=True, Y = X).
# The paths hold fp32 values (the C oracle rounds its inputs to fp32); fp64 I/O returns K unrounded, fp32 I/O once.
F64, F32 = torch.float64, torch.float32
CASES = [
    (3, 4, 300, 3, 0, 0, False, F64, "rand"),
    (2, 3, 1024, 2, 0, 0, False, F64, "ones"),
    (2, 2, 200, 4, 2, 0, False, F64, "sym"),
    (2, 2, 300, 2, 0, 0, True, F64, "ones"),
    (3, 3, 257, 5, 0, 1, False, F64, "ones"),
    (3, 4, 300, 3, 0, 0, False, F32, "ones"),
]


@pytest.mark.parametrize("A,B,T,d,n,kind,naive,io,weights", CASES)
def test_primitive_matches_oracle(gpu, A, B, T, d, n, kind, naive, io, weights):
    from sigsvgd_amd import ops

    rng = np.random.default_rng(A * 100 + T + n + kind)
    h = 0.5
    X = paths(rng, A, T, d)
    Y = X.copy() if weights == "sym" else paths(rng, B, T, d)
    if kind == 0:  # (the coverage kernel still takes the linear case's 257 points; the long route must agree there too)
        assert not ops.gram_takes(A, B, T, d, n, kind, True, naive, weights == "sym")
    go = rng.uniform(0.5, 1.5, (A, B)) if weights == "rand" else None
    go_ref = go if weights != "sym" else np.full((A, B), 2.0)
    Kr, gr = c_oracle.gram_fwd_bwd(X, Y, h=h, n=n, naive=naive, kind=kind, grad_out=go_ref)
    Xt, Yt = torch.as_tensor(X, dtype=io, device=gpu), torch.as_tensor(Y, dtype=io, device=gpu)
    got = None if go is None else torch.as_tensor(go, device=gpu)
    K, gX = ops.gram_long_fwd_bwd(Xt, Yt, 1.0 / h, n, kind, got, naive, sym=weights == "sym")
    assert K.dtype == io and gX.dtype == io and gX.shape == Xt.shape
    assert relK(np64(K), Kr) < (1e-9 if io == F64 else 2.0**-23)  # (fp32 I/O: K within its one rounding to fp32)
    assert relmax(np64(gX), gr) < 1e-5
    K2 = ops.gram_long_fwd(Xt, Yt, 1.0 / h, n, kind, naive)
    assert torch.equal(K, K2)


def test_refined_edge_8192(gpu):
    """P = Q = 8192 (129 points at order 6): the long route and the user route (sig_pde, which shares its sweeps) against
    each other and each against the C oracle (two 8193^2 fp64 tables per oracle thread: two threads)."""
    import sigsvgd_amd.sigkernel as sk
    from sigsvgd_amd import ops

    rng = np.random.default_rng(8192)
    Xn, Yn = paths(rng, 1, 129, 2), paths(rng, 2, 129, 2)
    X = torch.as_tensor(Xn, dtype=torch.float64, device=gpu)
    Y = torch.as_tensor(Yn, dtype=torch.float64, device=gpu)
    W = torch.tensor([[0.7, 1.3]], dtype=torch.float64, device=gpu)
    K, gX = ops.gram_long_fwd_bwd(X, Y, 1.0, 6, 0, W)
    Ku, gu = sk.SigKernel(DisguisedRBF(1.0), 6).gram_and_grad(X, Y, W)
    assert relK(np64(K), np64(Ku)) < 1e-9
    assert relmax(np64(gX), np64(gu)) < 1e-5
    Kr, gr = c_oracle.gram_fwd_bwd(Xn, Yn, h=1.0, n=6, grad_out=np64(W), nthreads=2)
    assert relK(np64(K), Kr) < 1e-9 and relK(np64(Ku), Kr) < 1e-9
    assert relmax(np64(gX), gr) < 1e-5 and relmax(np64(gu), gr) < 1e-5


def test_unequal_lengths(gpu):
    """X [3, 400, 2] against Y [4, 150, 2] at their own lengths; the oracle takes Y padded with its last point (exact)."""
    from sigsvgd_amd import ops

    rng = np.random.default_rng(11)
    X, Y = paths(rng, 3, 400, 2), paths(rng, 4, 150, 2)
    Ypad = np.concatenate([Y, np.repeat(Y[:, -1:], 400 - 150, axis=1)], axis=1)
    go = rng.uniform(0.5, 1.5, (3, 4))
    Kr, gr = c_oracle.gram_fwd_bwd(X, Ypad, h=1.0, n=0, grad_out=go)
    K, gX = ops.gram_long_fwd_bwd(torch.as_tensor(X, dtype=F64, device=gpu), torch.as_tensor(Y, dtype=F64, device=gpu), 1.0,
                                  0, 0, torch.as_tensor(go, device=gpu))
    assert K.shape == (3, 4) and gX.shape == (3, 400, 2)
    assert relK(np64(K), Kr) < 1e-9
    assert relmax(np64(gX), gr) < 1e-5


@pytest.mark.parametrize("T,d,n,kind", [(100, 3, 0, 0), (20, 2, 3, 0), (60, 3, 1, 1)])
def test_overlap_with_coverage_kernel(gpu, T, d, n, kind):
    """Where the coverage kernel also runs (fp64 end to end with force_generic), the two routes agree."""
    from sigsvgd_amd import ops

    rng = np.random.default_rng(T + n)
    X = torch.as_tensor(paths(rng, 4, T, d), dtype=F64, device=gpu)
    Y = torch.as_tensor(paths(rng, 5, T, d), dtype=F64, device=gpu)
    go = torch.as_tensor(rng.uniform(0.5, 1.5, (4, 5)), device=gpu)
    Kg, gg = ops.gram_fwd_bwd(X, Y, 2.0, n, kind, go, force_generic=True)
    Kl, gl = ops.gram_long_fwd_bwd(X, Y, 2.0, n, kind, go)
    assert relK(np64(Kl), np64(Kg)) < 1e-9
    assert relmax(np64(gl), np64(gg)) < 1e-5


def _surface_inputs(gpu, A=4, T=300, d=3, seed=5):
    rng = np.random.default_rng(seed)
    X = torch.as_tensor(paths(rng, A, T, d), dtype=torch.float64, device=gpu)
    Y = torch.as_tensor(paths(rng, A, T, d), dtype=torch.float64, device=gpu)
    W = torch.as_tensor(rng.uniform(0.5, 1.5, (A, A)), device=gpu)
    return X, Y, W


def _gram_and_xgrad(kernel, X, Y, W, sym):
    Xg = X.detach().clone().requires_grad_(True)
    K = kernel.compute_Gram(Xg, Xg if sym else Y, sym=sym)
    loss = K.sum() if W is None else (K * W).sum()
    (gX,) = torch.autograd.grad(loss, Xg)
    return K.detach(), gX


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("sym", [False, True])
def test_compute_gram_matches_user_route(gpu, sym, weighted):
    import sigsvgd_amd.sigkernel as sk
    from sigsvgd_amd import ops

    X, Y, W = _surface_inputs(gpu)
    assert not ops.gram_takes(4, 4, 300, 3, 0)
    Kb, gb = _gram_and_xgrad(sk.SigKernel(sk.RBFKernel(0.8), 0), X, Y, W if weighted else None, sym)
    Ku, gu = _gram_and_xgrad(sk.SigKernel(DisguisedRBF(0.8), 0), X, Y, W if weighted else None, sym)
    assert relK(np64(Kb), np64(Ku)) < 1e-9
    assert relmax(np64(gb), np64(gu)) < 1e-5


def test_gram_and_grad_and_mmd_match_user_route(gpu):
    import sigsvgd_amd.sigkernel as sk

    X, Y, W = _surface_inputs(gpu, T=200, seed=6)
    kb, ku = sk.SigKernel(sk.RBFKernel(1.0), 2), sk.SigKernel(DisguisedRBF(1.0), 2)  # P = 796: refused by the fused route
    for (Yv, sym) in [(Y, False), (None, True)]:
        Kb, gb = kb.gram_and_grad(X, Yv, W, sym=sym)
        Ku, gu = ku.gram_and_grad(X, Yv, W, sym=sym)
        assert relK(np64(Kb), np64(Ku)) < 1e-9 and relmax(np64(gb), np64(gu)) < 1e-5
    mb, mu = float(kb.compute_mmd(X, Y)), float(ku.compute_mmd(X, Y))
    assert abs(mb - mu) < 1e-9 * max(1.0, abs(mu))
    db, du = float(kb.compute_distance(X, Y)), float(ku.compute_distance(X, Y))
    assert abs(db - du) < 1e-9 * max(1.0, abs(du))


def test_svgd_step_with_signature_kernel(gpu):
    import sigsvgd_amd.sigkernel as sk
    from sigsvgd_amd.inference import SVGD
    from sigsvgd_amd.kernels import SignatureKernel

    rng = np.random.default_rng(2)
    X = torch.as_tensor(paths(rng, 8, 300, 3), dtype=torch.float64, device=gpu)  # (fp64: the user route's grid too)
    score = torch.as_tensor(rng.standard_normal((8, 300, 3)), dtype=torch.float64, device=gpu)
    out = []
    for kernel in (SignatureKernel(lambda _: 2.0, depth=0), sk.SigKernel(DisguisedRBF(2.0), 0)):
        s = SVGD(kernel, optimizer_class=None, lr=0.05)
        Xn, info = s.step(X.clone(), score)
        out.append((np64(Xn), np64(info["grad"])))
    assert relmax(out[0][0], out[1][0]) < 1e-5 and relmax(out[0][1], out[1][1]) < 1e-5


def test_long_determinism(gpu):
    from sigsvgd_amd import ops

    rng = np.random.default_rng(1)
    for (A, B, T, n) in [(5, 7, 300, 0), (3, 3, 100, 3)]:
        X = torch.as_tensor(paths(rng, A, T, 2), device=gpu)
        Y = torch.as_tensor(paths(rng, B, T, 2), device=gpu)
        go = torch.as_tensor(rng.standard_normal((A, B)), device=gpu)
        K1, g1 = ops.gram_long_fwd_bwd(X, Y, 1.0, n, 0, go)
        K2, g2 = ops.gram_long_fwd_bwd(X, Y, 1.0, n, 0, go)
        assert torch.equal(K1, K2) and torch.equal(g1, g2)


def test_forward_memory_stays_small(gpu):
    """A = B = 16 paths of 2048 points: the grid the user route builds would be 8.6 GB in fp64; the long route keeps it
    inside the kernel."""
    import sigsvgd_amd.sigkernel as sk

    rng = np.random.default_rng(3)
    X = torch.as_tensor(paths(rng, 16, 2048, 2), dtype=torch.float64, device=gpu)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(gpu)
    base = torch.cuda.memory_allocated(gpu)
    K = sk.SigKernel(sk.RBFKernel(1.0), 0).compute_Gram(X, X)
    torch.cuda.synchronize()
    assert K.shape == (16, 16) and bool(torch.isfinite(K).all())
    assert torch.cuda.max_memory_allocated(gpu) - base < (2 << 30)
    assert relK(np64(K), np64(K.T)) < 1e-9  # (each ordered pair is solved: K is symmetric to rounding)


# ---- the plan's branches (tests/helpers.long_plan mirrors long_make_plan; test_long_cabi.py pins it to the library) ------
def oracle_at_own_lengths(X, Y, h, n, naive, kind, go, nthreads=0):
    """The C oracle for X [A, TX, d] x Y [B, TY, d]: the shorter batch padded with its last point (exact,
    `ops.pad_to_length`), the gradient of a padded X folded back onto its points (`ops.fold_padded_grad`)."""
    from sigsvgd_amd import ops

    T = max(X.shape[1], Y.shape[1])
    pad = lambda P: ops.pad_to_length(torch.as_tensor(P), T).numpy()
    Kr, gr = c_oracle.gram_fwd_bwd(pad(X), pad(Y), h=h, n=n, naive=naive, kind=kind, grad_out=go, nthreads=nthreads)
    return Kr, ops.fold_padded_grad(torch.as_tensor(gr), X.shape[1]).numpy()


def _regime(tag, pl, M, N):
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


def _branch_id(c):
    A, B, TX, TY, d, n, kind, naive, reg = c
    return f"{reg}-{A}x{B}-T{TX}x{TY}-d{d}-n{n}-{'lin' if kind else 'rbf'}{'-naive' if naive else ''}"


@pytest.mark.parametrize("A,B,TX,TY,d,n,kind,naive,regime", BRANCH_CASES, ids=[_branch_id(c) for c in BRANCH_CASES])
def test_plan_branches_match_oracle(gpu, A, B, TX, TY, d, n, kind, naive, regime):
    from helpers import device_cus, long_plan
    from sigsvgd_amd import ops

    pl = long_plan(A, B, TX, TY, d, n, True, device_cus())
    assert pl is not None and _regime(regime, pl, TX, TY), pl
    rng = np.random.default_rng(TX * 7 + TY + 100 * d + n + 13 * kind)
    h = 0.5
    X, Y = paths(rng, A, TX, d, d**-0.5), paths(rng, B, TY, d, d**-0.5)
    go = rng.uniform(0.5, 1.5, (A, B))
    Kr, gr = oracle_at_own_lengths(X, Y, h, n, naive, kind, go, nthreads=2 if max(pl["P"], pl["Q"]) > 4096 else 0)
    Xt, Yt = torch.as_tensor(X, dtype=F64, device=gpu), torch.as_tensor(Y, dtype=F64, device=gpu)
    K, gX = ops.gram_long_fwd_bwd(Xt, Yt, 1.0 / h, n, kind, torch.as_tensor(go, device=gpu), naive)
    assert K.shape == (A, B) and gX.shape == Xt.shape
    assert relK(np64(K), Kr) < 1e-9
    assert relmax(np64(gX), gr) < 1e-5
    assert torch.equal(ops.gram_long_fwd(Xt, Yt, 1.0 / h, n, kind, naive), K)


@pytest.mark.parametrize("A,B,weights,io", [(64, 64, "rand", F64), (40, 60, "rand", F64), (64, 64, "sym", F64),
                                            (64, 64, "sym", F32)])
def test_work_items_with_several_pairs(gpu, A, B, weights, io):
    """Work items of JC > 1 pairs (the in-slab accumulation of a row's gradient over j) and more items than resident waves
    (the persistent item loop), with non-uniform weights, and sym=True (weights w_ij + w_ji) in fp64 and fp32 I/O."""
    from helpers import device_cus, long_plan
    from sigsvgd_amd import ops

    T, d, n, h = 40, 2, 0, 0.5
    pl = long_plan(A, B, T, T, d, n, True, device_cus())
    assert pl["JC"] > 1, pl
    if (A, B) == (40, 60):
        assert pl["items"] > pl["grid"], pl
    rng = np.random.default_rng(A + B + (weights == "sym") + (io == F32))
    X = paths(rng, A, T, d)
    Y = X.copy() if weights == "sym" else paths(rng, B, T, d)
    go = rng.uniform(0.5, 1.5, (A, B))
    Kr, gr = c_oracle.gram_fwd_bwd(X, Y, h=h, n=n, grad_out=go + go.T if weights == "sym" else go)
    Xt, Yt = torch.as_tensor(X, dtype=io, device=gpu), torch.as_tensor(Y, dtype=io, device=gpu)
    K, gX = ops.gram_long_fwd_bwd(Xt, Yt, 1.0 / h, n, 0, torch.as_tensor(go, device=gpu), sym=weights == "sym")
    assert K.dtype == io and gX.dtype == io
    assert relK(np64(K), Kr) < (1e-9 if io == F64 else 2.0**-23)
    assert relmax(np64(gX), gr) < 1e-5
