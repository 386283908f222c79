"""Long paths with the built-in static kernels (csrc/gram_long.hip, `ops.gram_long_*`, the routing of
`sigsvgd_amd.sigkernel`): against the C oracle, against the coverage kernel where both run, and against the user
static-kernel route (`DisguisedRBF`: the same RBF behind upstream's interface, solved by csrc/sig_pde.hip on the grid torch
builds).  Every RBF shape here except the overlap cases is one the fused Gram kernels refuse for LDS."""
import numpy as np
import pytest
import torch

from oracle import c_oracle
from parity import DisguisedRBF, gram_and_xgrad, np64, rel_entry, rel_max, sized_walks
from plans import BRANCH_CASES, branch_id, branch_regime, device_cus, long_plan, oracle_at_own_lengths

pytestmark = pytest.mark.gpu


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
    X = sized_walks(rng, A, T, d)
    Y = X.copy() if weights == "sym" else sized_walks(rng, B, T, d)
    if kind == 0:  # (the coverage kernel still takes the linear case's 257 points; the long route must agree there too)
        assert not ops.gram_takes(A, B, T, d, n, kind, True, naive, weights == "sym")
    go = rng.uniform(0.5, 1.5, (A, B)) if weights == "rand" else None
    go_ref = go if weights != "sym" else np.full((A, B), 2.0)
    Kr, gr = c_oracle.gram_fwd_bwd(X, Y, h=h, n=n, naive=naive, kind=kind, grad_out=go_ref)
    Xt, Yt = torch.as_tensor(X, dtype=io, device=gpu), torch.as_tensor(Y, dtype=io, device=gpu)
    got = None if go is None else torch.as_tensor(go, device=gpu)
    K, gX = ops.gram_long_fwd_bwd(Xt, Yt, 1.0 / h, n, kind, got, naive, sym=weights == "sym")
    assert K.dtype == io and gX.dtype == io and gX.shape == Xt.shape
    assert rel_entry(np64(K), Kr, 0.0) < (1e-9 if io == F64 else 2.0**-23)  # (fp32 I/O: K within its one rounding to fp32)
    assert rel_max(np64(gX), gr) < 1e-5
    K2 = ops.gram_long_fwd(Xt, Yt, 1.0 / h, n, kind, naive)
    assert torch.equal(K, K2)


def test_refined_edge_8192(gpu):
    """P = Q = 8192 (129 points at order 6): the long route and the user route (sig_pde, which shares its sweeps) against
    each other and each against the C oracle (two 8193^2 fp64 tables per oracle thread: two threads)."""
    import sigsvgd_amd.sigkernel as sk
    from sigsvgd_amd import ops

    rng = np.random.default_rng(8192)
    Xn, Yn = sized_walks(rng, 1, 129, 2), sized_walks(rng, 2, 129, 2)
    X = torch.as_tensor(Xn, dtype=torch.float64, device=gpu)
    Y = torch.as_tensor(Yn, dtype=torch.float64, device=gpu)
    W = torch.tensor([[0.7, 1.3]], dtype=torch.float64, device=gpu)
    K, gX = ops.gram_long_fwd_bwd(X, Y, 1.0, 6, 0, W)
    Ku, gu = sk.SigKernel(DisguisedRBF(1.0), 6).gram_and_grad(X, Y, W)
    assert rel_entry(np64(K), np64(Ku), 0.0) < 1e-9
    assert rel_max(np64(gX), np64(gu)) < 1e-5
    Kr, gr = c_oracle.gram_fwd_bwd(Xn, Yn, h=1.0, n=6, grad_out=np64(W), nthreads=2)
    assert rel_entry(np64(K), Kr, 0.0) < 1e-9 and rel_entry(np64(Ku), Kr, 0.0) < 1e-9
    assert rel_max(np64(gX), gr) < 1e-5 and rel_max(np64(gu), gr) < 1e-5


def test_unequal_lengths(gpu):
    """X [3, 400, 2] against Y [4, 150, 2] at their own lengths; the oracle takes Y padded with its last point (exact)."""
    from sigsvgd_amd import ops

    rng = np.random.default_rng(11)
    X, Y = sized_walks(rng, 3, 400, 2), sized_walks(rng, 4, 150, 2)
    Ypad = np.concatenate([Y, np.repeat(Y[:, -1:], 400 - 150, axis=1)], axis=1)
    go = rng.uniform(0.5, 1.5, (3, 4))
    Kr, gr = c_oracle.gram_fwd_bwd(X, Ypad, h=1.0, n=0, grad_out=go)
    K, gX = ops.gram_long_fwd_bwd(torch.as_tensor(X, dtype=F64, device=gpu), torch.as_tensor(Y, dtype=F64, device=gpu), 1.0,
                                  0, 0, torch.as_tensor(go, device=gpu))
    assert K.shape == (3, 4) and gX.shape == (3, 400, 2)
    assert rel_entry(np64(K), Kr, 0.0) < 1e-9
    assert rel_max(np64(gX), gr) < 1e-5


@pytest.mark.parametrize("T,d,n,kind", [(100, 3, 0, 0), (20, 2, 3, 0), (60, 3, 1, 1)])
def test_overlap_with_coverage_kernel(gpu, T, d, n, kind):
    """Where the coverage kernel also runs (fp64 end to end with force_generic), the two routes agree."""
    from sigsvgd_amd import ops

    rng = np.random.default_rng(T + n)
    X = torch.as_tensor(sized_walks(rng, 4, T, d), dtype=F64, device=gpu)
    Y = torch.as_tensor(sized_walks(rng, 5, T, d), dtype=F64, device=gpu)
    go = torch.as_tensor(rng.uniform(0.5, 1.5, (4, 5)), device=gpu)
    Kg, gg = ops.gram_fwd_bwd(X, Y, 2.0, n, kind, go, force_generic=True)
    Kl, gl = ops.gram_long_fwd_bwd(X, Y, 2.0, n, kind, go)
    assert rel_entry(np64(Kl), np64(Kg), 0.0) < 1e-9
    assert rel_max(np64(gl), np64(gg)) < 1e-5


def _surface_inputs(gpu, A=4, T=300, d=3, seed=5):
    rng = np.random.default_rng(seed)
    X = torch.as_tensor(sized_walks(rng, A, T, d), dtype=torch.float64, device=gpu)
    Y = torch.as_tensor(sized_walks(rng, A, T, d), dtype=torch.float64, device=gpu)
    W = torch.as_tensor(rng.uniform(0.5, 1.5, (A, A)), device=gpu)
    return X, Y, W


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("sym", [False, True])
def test_compute_gram_matches_user_route(gpu, sym, weighted):
    import sigsvgd_amd.sigkernel as sk
    from sigsvgd_amd import ops

    X, Y, W = _surface_inputs(gpu)
    assert not ops.gram_takes(4, 4, 300, 3, 0)
    Kb, gb = gram_and_xgrad(sk.SigKernel(sk.RBFKernel(0.8), 0), X, Y, W if weighted else None, sym)
    Ku, gu = gram_and_xgrad(sk.SigKernel(DisguisedRBF(0.8), 0), X, Y, W if weighted else None, sym)
    assert rel_entry(np64(Kb), np64(Ku), 0.0) < 1e-9
    assert rel_max(np64(gb), np64(gu)) < 1e-5


def test_gram_and_grad_and_mmd_match_user_route(gpu):
    import sigsvgd_amd.sigkernel as sk

    X, Y, W = _surface_inputs(gpu, T=200, seed=6)
    kb, ku = sk.SigKernel(sk.RBFKernel(1.0), 2), sk.SigKernel(DisguisedRBF(1.0), 2)  # P = 796: refused by the fused route
    for (Yv, sym) in [(Y, False), (None, True)]:
        Kb, gb = kb.gram_and_grad(X, Yv, W, sym=sym)
        Ku, gu = ku.gram_and_grad(X, Yv, W, sym=sym)
        assert rel_entry(np64(Kb), np64(Ku), 0.0) < 1e-9 and rel_max(np64(gb), np64(gu)) < 1e-5
    mb, mu = float(kb.compute_mmd(X, Y)), float(ku.compute_mmd(X, Y))
    assert abs(mb - mu) < 1e-9 * max(1.0, abs(mu))
    db, du = float(kb.compute_distance(X, Y)), float(ku.compute_distance(X, Y))
    assert abs(db - du) < 1e-9 * max(1.0, abs(du))


def test_svgd_step_with_signature_kernel(gpu):
    import sigsvgd_amd.sigkernel as sk
    from sigsvgd_amd.inference import SVGD
    from sigsvgd_amd.kernels import SignatureKernel

    rng = np.random.default_rng(2)
    X = torch.as_tensor(sized_walks(rng, 8, 300, 3), dtype=torch.float64, device=gpu)  # (fp64: the user route's grid too)
    score = torch.as_tensor(rng.standard_normal((8, 300, 3)), dtype=torch.float64, device=gpu)
    out = []
    for kernel in (SignatureKernel(lambda _: 2.0, depth=0), sk.SigKernel(DisguisedRBF(2.0), 0)):
        s = SVGD(kernel, optimizer_class=None, lr=0.05)
        Xn, info = s.step(X.clone(), score)
        out.append((np64(Xn), np64(info["grad"])))
    assert rel_max(out[0][0], out[1][0]) < 1e-5 and rel_max(out[0][1], out[1][1]) < 1e-5


def test_long_determinism(gpu):
    from sigsvgd_amd import ops

    rng = np.random.default_rng(1)
    for (A, B, T, n) in [(5, 7, 300, 0), (3, 3, 100, 3)]:
        X = torch.as_tensor(sized_walks(rng, A, T, 2), device=gpu)
        Y = torch.as_tensor(sized_walks(rng, B, T, 2), device=gpu)
        go = torch.as_tensor(rng.standard_normal((A, B)), device=gpu)
        K1, g1 = ops.gram_long_fwd_bwd(X, Y, 1.0, n, 0, go)
        K2, g2 = ops.gram_long_fwd_bwd(X, Y, 1.0, n, 0, go)
        assert torch.equal(K1, K2) and torch.equal(g1, g2)


def test_forward_memory_stays_small(gpu):
    """A = B = 16 paths of 2048 points: the grid the user route builds would be 8.6 GB in fp64; the long route keeps it
    inside the kernel."""
    import sigsvgd_amd.sigkernel as sk

    rng = np.random.default_rng(3)
    X = torch.as_tensor(sized_walks(rng, 16, 2048, 2), dtype=torch.float64, device=gpu)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(gpu)
    base = torch.cuda.memory_allocated(gpu)
    K = sk.SigKernel(sk.RBFKernel(1.0), 0).compute_Gram(X, X)
    torch.cuda.synchronize()
    assert K.shape == (16, 16) and bool(torch.isfinite(K).all())
    assert torch.cuda.max_memory_allocated(gpu) - base < (2 << 30)
    assert rel_entry(np64(K), np64(K.T), 0.0) < 1e-9  # (each ordered pair is solved: K is symmetric to rounding)


# ---- the plan's branches (tests/plans.long_plan mirrors long_make_plan; test_long_cabi.py pins it to the library) ------
# (A, B, TX, TY, d, n, kind, naive, regime); nthreads of the oracle where its tables are large
@pytest.mark.parametrize("A,B,TX,TY,d,n,kind,naive,regime", BRANCH_CASES, ids=[branch_id(c) for c in BRANCH_CASES])
def test_plan_branches_match_oracle(gpu, A, B, TX, TY, d, n, kind, naive, regime):
    from sigsvgd_amd import ops

    pl = long_plan(A, B, TX, TY, d, n, True, device_cus())
    assert pl is not None and branch_regime(regime, pl, TX, TY), pl
    rng = np.random.default_rng(TX * 7 + TY + 100 * d + n + 13 * kind)
    h = 0.5
    X, Y = sized_walks(rng, A, TX, d, d**-0.5), sized_walks(rng, B, TY, d, d**-0.5)
    go = rng.uniform(0.5, 1.5, (A, B))
    Kr, gr = oracle_at_own_lengths(X, Y, h, n, naive, kind, go, nthreads=2 if max(pl["P"], pl["Q"]) > 4096 else 0)
    Xt, Yt = torch.as_tensor(X, dtype=F64, device=gpu), torch.as_tensor(Y, dtype=F64, device=gpu)
    K, gX = ops.gram_long_fwd_bwd(Xt, Yt, 1.0 / h, n, kind, torch.as_tensor(go, device=gpu), naive)
    assert K.shape == (A, B) and gX.shape == Xt.shape
    assert rel_entry(np64(K), Kr, 0.0) < 1e-9
    assert rel_max(np64(gX), gr) < 1e-5
    assert torch.equal(ops.gram_long_fwd(Xt, Yt, 1.0 / h, n, kind, naive), K)


@pytest.mark.parametrize("A,B,weights,io", [(64, 64, "rand", F64), (40, 60, "rand", F64), (64, 64, "sym", F64),
                                            (64, 64, "sym", F32)])
def test_work_items_with_several_pairs(gpu, A, B, weights, io):
    """Work items of JC > 1 pairs (the in-slab accumulation of a row's gradient over j) and more items than resident waves
    (the persistent item loop), with non-uniform weights, and sym=True (weights w_ij + w_ji) in fp64 and fp32 I/O."""
    from sigsvgd_amd import ops

    T, d, n, h = 40, 2, 0, 0.5
    pl = long_plan(A, B, T, T, d, n, True, device_cus())
    assert pl["JC"] > 1, pl
    if (A, B) == (40, 60):
        assert pl["items"] > pl["grid"], pl
    rng = np.random.default_rng(A + B + (weights == "sym") + (io == F32))
    X = sized_walks(rng, A, T, d)
    Y = X.copy() if weights == "sym" else sized_walks(rng, B, T, d)
    go = rng.uniform(0.5, 1.5, (A, B))
    Kr, gr = c_oracle.gram_fwd_bwd(X, Y, h=h, n=n, grad_out=go + go.T if weights == "sym" else go)
    Xt, Yt = torch.as_tensor(X, dtype=io, device=gpu), torch.as_tensor(Y, dtype=io, device=gpu)
    K, gX = ops.gram_long_fwd_bwd(Xt, Yt, 1.0 / h, n, 0, torch.as_tensor(go, device=gpu), sym=weights == "sym")
    assert K.dtype == io and gX.dtype == io
    assert rel_entry(np64(K), Kr, 0.0) < (1e-9 if io == F64 else 2.0**-23)
    assert rel_max(np64(gX), gr) < 1e-5
