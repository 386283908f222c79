"""GPU parity across regimes: rough / smooth paths, small / large bandwidths, degenerate paths, on all three
solvers (register-resident T <= 64, streaming T <= 128, coverage).  Tolerance 1e-5 relative to max-abs
(BASELINE.json north_star), fp32 I/O against the fp64 C oracle."""
import numpy as np
import pytest
import torch

from oracle import c_oracle as C
from parity import rel_entry, rel_max, walks

pytestmark = pytest.mark.gpu
TOL = 1e-5


@pytest.mark.parametrize("T,d", [(64, 7), (33, 3), (128, 14), (96, 5)])
@pytest.mark.parametrize("scale,h", [(0.01, 1.0), (0.05, 0.1), (0.05, 10.0), (0.15, 1.0), (0.3, 4.0), (0.02, 0.02)])
def test_regimes_self_gram(gpu, T, d, scale, h):
    """Y is X (the SVGD call): includes the diagonal pairs, whose K can reach 1e3 for rough paths"""
    from sigsvgd_amd import ops

    N = 10
    X = walks(N, T, d, 21, scale)
    Kref, gref = C.gram_fwd_bwd(X, X, h, 0)
    if not np.isfinite(Kref).all() or Kref.max() > 1e30:
        pytest.skip("regime overflows the oracle")
    Xg = torch.as_tensor(X, device=gpu)
    K, g = ops.gram_fwd_bwd(Xg, Xg, 1.0 / h, y_is_x=True)
    Ko, go_ = ops.gram_fwd_bwd(Xg, Xg.clone(), 1.0 / h)
    assert torch.isfinite(K).all() and torch.isfinite(g).all()
    assert rel_entry(K.cpu().numpy(), Kref, 1e-6) < TOL, ("K sym", Kref.max())
    assert rel_entry(Ko.cpu().numpy(), Kref, 1e-6) < TOL, ("K ordered", Kref.max())
    assert rel_max(g.cpu().numpy(), gref) < TOL, ("grad sym", Kref.max(), np.abs(gref).max())
    assert rel_max(go_.cpu().numpy(), gref) < TOL, ("grad ordered", Kref.max(), np.abs(gref).max())


@pytest.mark.parametrize("T,d,n", [(20, 2, 2), (10, 3, 4), (30, 2, 3)])
@pytest.mark.parametrize("scale,h", [(0.05, 1.0), (0.3, 5.0), (0.1, 0.2)])
def test_regimes_coverage_kernel(gpu, T, d, n, scale, h):
    from sigsvgd_amd import ops

    X, Y = walks(6, T, d, 31, scale), walks(7, T, d, 32, scale)
    Kref, gref = C.gram_fwd_bwd(X, Y, h, n)
    K, g = ops.gram_fwd_bwd(torch.as_tensor(X, device=gpu), torch.as_tensor(Y, device=gpu), 1.0 / h, n)
    assert rel_entry(K.cpu().numpy(), Kref, 1e-6) < TOL and rel_max(g.cpu().numpy(), gref) < TOL


@pytest.mark.parametrize("T,d", [(64, 7), (128, 14), (40, 2)])
def test_degenerate_paths(gpu, T, d):
    """constant paths (all increments zero): K = 1 exactly and a vanishing gradient; a path against itself
    repeated: K symmetric with equal rows; duplicated consecutive points change nothing (g = 0 cells)."""
    from sigsvgd_amd import ops

    const = np.tile(np.random.default_rng(1).standard_normal((3, 1, d)).astype(np.float32), (1, T, 1))
    mov = walks(4, T, d, 2, 0.05)
    K, g = ops.gram_fwd_bwd(torch.as_tensor(const, device=gpu), torch.as_tensor(mov, device=gpu), 1.0)
    assert torch.equal(K, torch.ones_like(K))
    K2, g2 = ops.gram_fwd_bwd(torch.as_tensor(mov, device=gpu), torch.as_tensor(const, device=gpu), 1.0)
    # (constant column paths: the true gradient is 0; the fp32 contraction of R G (x - y) leaves one rounding of a
    #  product of order |x - y|, i.e. 1e-8 where gradients of moving pairs are of order 1)
    assert torch.equal(K2, torch.ones_like(K2)) and float(g2.abs().max()) < 2e-7
    same = np.repeat(mov[:1], 5, axis=0)
    K3, g3 = ops.gram_fwd_bwd(torch.as_tensor(same, device=gpu), torch.as_tensor(same, device=gpu), 1.0, y_is_x=True)
    assert float((K3 - K3[0, 0]).abs().max()) <= 1e-6 * float(K3[0, 0])
    # (identical rows up to the order of the fp32 column-side sums)
    assert rel_max(g3[1:].cpu().numpy(), g3[:1].double().cpu().numpy().repeat(4, 0)) < 3e-6
    # a repeated point: path of length T with x[t] == x[t+1] at one place vs the oracle
    rep = mov.copy()
    rep[:, T // 2] = rep[:, T // 2 - 1]
    Kref, gref = C.gram_fwd_bwd(rep, mov, 1.0, 0)
    K4, g4 = ops.gram_fwd_bwd(torch.as_tensor(rep, device=gpu), torch.as_tensor(mov, device=gpu), 1.0)
    assert rel_entry(K4.cpu().numpy(), Kref, 1e-6) < TOL and rel_max(g4.cpu().numpy(), gref) < TOL


@pytest.mark.parametrize("T,d,n,generic", [(64, 7, 0, False), (32, 2, 0, False), (100, 5, 0, False), (20, 2, 2, False),
                                           (10, 2, 4, False), (64, 7, 0, True), (10, 2, 4, True)])
def test_non_finite_inputs_propagate_without_hanging(gpu, T, d, n, generic):
    """a NaN in one trajectory poisons its own row/column only; the launch completes -- on every pair kernel (the fp64 pass
    over flagged pairs must not turn a NaN pair into a number: NaN pairs are not flagged, and the coverage kernel's
    exponential hands a NaN through)"""
    from sigsvgd_amd import ops

    X = walks(9, T, d, 5, 0.05)
    X[3, min(10, T - 2), d - 1] = np.nan
    Xg = torch.as_tensor(X, device=gpu)
    K, g = ops.gram_fwd_bwd(Xg, Xg, 1.0, n, y_is_x=True, force_generic=generic)
    Kf = ops.gram_fwd(Xg, Xg.clone(), 1.0, n, force_generic=generic)
    torch.cuda.synchronize()
    for Kx in (K, Kf):
        bad = torch.isnan(Kx)
        assert bad[3].all() and bad[:, 3].all()
        ok = [i for i in range(9) if i != 3]
        assert torch.isfinite(Kx[ok][:, ok]).all()


def test_rough_long_paths_are_solved(gpu):
    """Long paths so rough that a path against itself has K ~ 1e13 and static-kernel increments near 1 (the kernel
    this build retired regenerated the forward solution backwards and had to decline such pairs with NaN gradients):
    every kernel now keeps the forward solution, so K and the gradient are simply right, at every path length."""
    from sigsvgd_amd import ops

    for (T, d, scale) in [(100, 7, 0.25), (128, 14, 0.15), (66, 3, 0.4), (128, 2, 0.5)]:
        X = walks(6, T, d, 21, scale)
        Kref, gref = C.gram_fwd_bwd(X, X, 1.0, 0)
        Xg = torch.as_tensor(X, device=gpu)
        K, g = ops.gram_fwd_bwd(Xg, Xg, 1.0, y_is_x=True)
        assert torch.isfinite(g).all()
        assert rel_entry(K.cpu().numpy(), Kref, 1e-6) < TOL and rel_max(g.cpu().numpy(), gref) < TOL, (T, d, float(Kref.max()))
        K2, g2 = ops.gram_fwd_bwd(Xg, Xg.clone(), 1.0)
        assert rel_entry(K2.cpu().numpy(), Kref, 1e-6) < TOL and rel_max(g2.cpu().numpy(), gref) < TOL
