"""GPU parity: the refined-grid kernels (gram_dyad.hip: short paths with dyadic refinement, refined grid of 64 .. 128 cells
per side -- the reference's own call shapes: examples/script_planning_obstacle_field.py:156-158,325 order 5 on 5 points,
script_planning_robot.py:391 order 6 on 3 points, BASELINE.json C1 order 2 on 20 points; gram_band.hip: 129 .. 256 cells --
examples/script_sequential_distribution.ipynb order 4 on 10 points, script_control_particle_maze.py:43-44 order 3 on 30
points) vs the fp64 oracle, via the C ABI."""
import numpy as np
import pytest
import torch

from oracle import c_oracle as C
from oracle import sigkernel_oracle as O
from parity import rel_entry, rel_max, walks

pytestmark = pytest.mark.gpu

TOL = 1e-5  # north_star tolerance (K per entry; gradients relative to max-abs)


# T, dyadic order, d  (refined cells per side = (T - 1) * 2^n)
SHAPES = [(20, 2, 2), (5, 5, 2), (3, 6, 7), (9, 3, 3), (17, 2, 14), (33, 2, 5), (10, 3, 16), (30, 2, 4), (5, 4, 8), (3, 5, 1)]
# the band kernel: 129 .. 256 cells (the notebook's and the maze script's shapes first; ragged last bands; 256 = the limit)
BAND_SHAPES = [(10, 4, 2), (30, 3, 2), (33, 3, 3), (18, 3, 14), (3, 7, 2), (20, 3, 7), (5, 6, 16), (27, 3, 1)]
SHAPES = SHAPES + BAND_SHAPES


def test_shapes_take_the_refined_grid_kernel():
    """the dispatch is a host-side predicate: cells per side in [64, 128] / (128, 256], at most 33 points"""
    for T, n, d in SHAPES:
        assert 64 <= (T - 1) << n <= 256 and T <= 33
    for T, n, d in BAND_SHAPES:
        assert 128 < (T - 1) << n


@pytest.mark.parametrize("T,n,d", SHAPES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_dyadic_general_xy(gpu, T, n, d, dtype):
    """X != Y, ragged batch sizes: ordered pairs, row-side gradient, arbitrary grad_out; equals the coverage kernel"""
    from sigsvgd_amd import ops

    A, B = 11, 9
    X, Y = walks(A, T, d, 1, 0.3), walks(B, T, d, 2, 0.3)
    h = 1.7
    go = np.random.default_rng(3).standard_normal((A, B)).astype(np.float32)
    Kref, gref = C.gram_fwd_bwd(X, Y, h, n, grad_out=go.astype(np.float64))
    Xg, Yg, gog = (torch.as_tensor(t, device=gpu).to(dtype) for t in (X, Y, go))
    K1 = ops.gram_fwd(Xg, Yg, 1.0 / h, n)
    K2, g2 = ops.gram_fwd_bwd(Xg, Yg, 1.0 / h, n, grad_out=gog)
    torch.cuda.synchronize()
    assert K2.dtype == dtype and g2.dtype == dtype
    assert rel_entry(K1.cpu().numpy(), Kref, 1e-6) < TOL and rel_entry(K2.cpu().numpy(), Kref, 1e-6) < TOL
    assert rel_max(g2.cpu().numpy(), gref) < TOL
    K3, g3 = ops.gram_fwd_bwd(Xg, Yg, 1.0 / h, n, grad_out=gog, force_generic=True)
    assert rel_entry(K2.cpu().numpy(), K3.double().cpu().numpy(), 1e-6) < TOL
    assert rel_max(g2.cpu().numpy(), g3.double().cpu().numpy()) < TOL


@pytest.mark.parametrize("T,n,d", SHAPES)
@pytest.mark.parametrize("weights", ["ones", "random", "sym"])
def test_dyadic_symmetric(gpu, T, n, d, weights):
    """Y is X: each unordered pair once, row- and column-side gradients; N = 19 leaves a last tile with three rows"""
    from sigsvgd_amd import ops

    N = 19
    X = walks(N, T, d, 5, 0.3)
    h = 0.9
    go, sym = None, False
    if weights != "ones":
        go = np.random.default_rng(7).standard_normal((N, N)).astype(np.float32)
    if weights == "sym":
        sym = True
    Kref, gref = O.gram_backward(X, X, None if go is None else go.astype(np.float64), O.RBF, h, n, False, sym)
    Xg = torch.as_tensor(X, device=gpu)
    gog = None if go is None else torch.as_tensor(go, device=gpu)
    K, g = ops.gram_fwd_bwd(Xg, Xg, 1.0 / h, n, grad_out=gog, sym=sym, y_is_x=True)
    torch.cuda.synchronize()
    Kn = K.cpu().numpy()
    assert rel_entry(Kn, Kref, 1e-6) < TOL and np.array_equal(Kn, Kn.T)
    assert rel_max(g.cpu().numpy(), gref) < TOL
    K2, g2 = ops.gram_fwd_bwd(Xg, Xg, 1.0 / h, n, grad_out=gog, sym=sym, y_is_x=True)
    assert torch.equal(K, K2) and torch.equal(g, g2)  # reproducible bits
    Kf = ops.gram_fwd(Xg, Xg, 1.0 / h, n, y_is_x=True)
    assert rel_entry(Kf.cpu().numpy(), Kref, 1e-6) < TOL


def test_refined_grid_kernel_large_launch(gpu, monkeypatch):
    """gram_dyad.hip with more items than workgroups (N = 300: 5,700 items of 8 rows), pinned to it: by default the
    band-parallel schedule of gram_band.hip takes every launch of 65 .. 128 cells"""
    from sigsvgd_amd import ops

    monkeypatch.setenv("SIGSVGD_BAND_MODE", "serial")
    N, T, d, n, h = 300, 5, 2, 5, 1.0
    X = walks(N, T, d, 12, 0.3)
    Xg = torch.as_tensor(X, device=gpu)
    K, g = ops.gram_fwd_bwd(Xg, Xg, 1.0 / h, n, y_is_x=True)
    Kref, gref = C.gram_fwd_bwd(X, X, h, n, rows=(0, 6))
    assert rel_entry(K.cpu().numpy()[:6], Kref, 1e-6) < TOL
    assert np.abs(g.cpu().numpy()[:6] - gref).max() / np.abs(g.cpu().numpy()).max() < TOL
    monkeypatch.setenv("SIGSVGD_BAND_MODE", "parallel")
    Kp, gp = ops.gram_fwd_bwd(Xg, Xg, 1.0 / h, n, y_is_x=True)
    assert rel_entry(Kp.cpu().numpy(), K.double().cpu().numpy(), 1e-6) < TOL and rel_max(gp.cpu().numpy(), g.double().cpu().numpy()) < TOL


def test_dyadic_reference_shapes_at_their_sizes(gpu):
    """the reference's planning experiment (30 particles x 5 knots in R^2, order 5) and BASELINE C1 (16 x 20 x 2, order 2)
    plus a launch with more items than workgroups (N = 300: 5,700 items); the notebook's experiment (100 x 10 x 2, order 4,
    bandwidth 5) and the maze controller's (35 policies x 30 steps x 2, order 3, sigma^2 = 32)"""
    from sigsvgd_amd import ops

    # (150 x 10, order 4: 11,325 pairs, more than five rounds of band-parallel workgroups -- the serial schedule by the
    #  launcher's own rule; the notebook and maze sizes take the band-parallel kernel)
    for N, T, d, n, h in [(30, 5, 2, 5, 0.9), (16, 20, 2, 2, 1.0), (300, 5, 2, 5, 1.0), (100, 10, 2, 4, 5.0), (35, 30, 2, 3, 5.6),
                          (150, 10, 2, 4, 5.0)]:
        X = walks(N, T, d, 11, 0.3)
        Xg = torch.as_tensor(X, device=gpu)
        K, g = ops.gram_fwd_bwd(Xg, Xg, 1.0 / h, n, y_is_x=True)
        rows = (0, min(N, 6))
        Kref, gref = C.gram_fwd_bwd(X, X, h, n, rows=rows)
        assert rel_entry(K.cpu().numpy()[rows[0]:rows[1]], Kref, 1e-6) < TOL
        gfull = np.abs(g.cpu().numpy()).max()
        assert np.abs(g.cpu().numpy()[rows[0]:rows[1]] - gref).max() / gfull < TOL
        Ko, go_ = ops.gram_fwd_bwd(Xg, Xg.clone(), 1.0 / h, n)
        # (two orientations of a pair: both within TOL of the oracle)
        assert rel_entry(Ko.cpu().numpy(), K.double().cpu().numpy(), 1e-6) < TOL
        assert rel_max(go_.cpu().numpy(), g.double().cpu().numpy()) < TOL


@pytest.mark.parametrize("T,n,d,scale,h,offset", [(30, 3, 2, 0.5, 3.0, 100.0), (30, 3, 2, 0.5, 1.0, 100.0), (30, 3, 2, 0.1, 0.1, 0.0),
                                                   (5, 6, 2, 0.02, 10.0, 100.0)])
def test_band_kernel_rough_and_smooth_extremes(gpu, T, n, d, scale, h, offset):
    """The band kernel's two accuracy mechanisms (gram_band.hip): pairs whose solution cancelled are flagged and solved again
    in fp64 by the coverage kernel (the maze shape in rough regimes: 1.4e-5 without), and at dyadic order >= 5 the
    full-magnitude add of the forward sweep runs in two floats (order 6, 256 cells, smooth paths: 1.2e-5 without)."""
    from sigsvgd_amd import ops

    X = walks(12, T, d, 0, scale=scale, offset=offset)
    Kref, gref = C.gram_fwd_bwd(X, X, h, n)
    Xg = torch.as_tensor(X, device=gpu)
    for K, g in [ops.gram_fwd_bwd(Xg, Xg, 1.0 / h, n, y_is_x=True), ops.gram_fwd_bwd(Xg, Xg.clone(), 1.0 / h, n)]:
        assert rel_entry(K.cpu().numpy(), Kref, 1e-6) < 5e-6
        assert rel_max(g.cpu().numpy(), gref) < TOL
    for K in [ops.gram_fwd(Xg, Xg, 1.0 / h, n, y_is_x=True), ops.gram_fwd(Xg, Xg.clone(), 1.0 / h, n)]:
        assert rel_entry(K.cpu().numpy(), Kref, 1e-6) < 5e-6


@pytest.mark.parametrize("T,n,d", BAND_SHAPES)
@pytest.mark.parametrize("sym", [True, False])
def test_band_kernels_agree(gpu, monkeypatch, T, n, d, sym):
    """gram_band.hip runs its kernel on two schedules for 129 .. 256 cells per side: a wavefront per pair that walks the bands
    in turn (launches with many pairs) and a wavefront per BAND of a pair, pipelined over a workgroup (the reference's sizes).
    Same arithmetic per cell and the same order in every block sum: K and the flags of the exact pass are equal bit for bit;
    the gradients differ by the order of the fixed-order reduction only (tiles of up to 8 rows against tiles of one).
    SIGSVGD_BAND_MODE picks the schedule."""
    _band_kernels_agree(gpu, monkeypatch, T, n, d, sym, 11)


@pytest.mark.parametrize("T,n", [(3, 7), (5, 6)])
@pytest.mark.parametrize("sym", [True, False])
def test_band_kernels_agree_wide_blocks(gpu, monkeypatch, T, n, sym):
    """the same at 64 and 128 fine cells per coarse cell, where a coarse cell's block sum spans a whole band or two (two
    wavefronts of the band-parallel schedule add into one cell), in a launch of three rows and two channels"""
    _band_kernels_agree(gpu, monkeypatch, T, n, 2, sym, 3)


def _band_kernels_agree(gpu, monkeypatch, T, n, d, sym, A):
    from sigsvgd_amd import ops

    B = A if sym else 7
    X = walks(A, T, d, 21, 0.2)
    Y = X if sym else walks(B, T, d, 22, 0.2)
    go = np.random.default_rng(3).uniform(0.5, 1.5, (A, B)).astype(np.float32)
    Kref, gref = C.gram_fwd_bwd(X, Y, 1.0, n, grad_out=go.astype(np.float64))
    Xg, gog = torch.as_tensor(X, device=gpu), torch.as_tensor(go, device=gpu)
    Yg = Xg if sym else torch.as_tensor(Y, device=gpu)
    res = {}
    for mode in ("serial", "parallel"):
        monkeypatch.setenv("SIGSVGD_BAND_MODE", mode)
        K, g = ops.gram_fwd_bwd(Xg, Yg, 1.0, n, grad_out=gog, y_is_x=sym)
        Kf = ops.gram_fwd(Xg, Yg, 1.0, n, y_is_x=sym)
        K2, g2 = ops.gram_fwd_bwd(Xg, Yg, 1.0, n, grad_out=gog, y_is_x=sym)
        torch.cuda.synchronize()
        assert torch.equal(K, K2) and torch.equal(g, g2)  # (reproducible, each of them)
        assert rel_entry(K.cpu().numpy(), Kref, 1e-6) < TOL and rel_entry(Kf.cpu().numpy(), Kref, 1e-6) < TOL
        assert rel_max(g.cpu().numpy(), gref) < TOL
        res[mode] = (K.cpu().numpy(), Kf.cpu().numpy(), g.cpu().numpy())
    assert np.array_equal(res["serial"][0], res["parallel"][0])
    assert np.array_equal(res["serial"][1], res["parallel"][1])
    assert rel_max(res["parallel"][2], res["serial"][2].astype(np.float64)) < 2e-6


@pytest.mark.parametrize("T,n,d", [s for s in SHAPES if 64 < (s[0] - 1) << s[1] <= 128 and s[1] >= 2])
@pytest.mark.parametrize("sym", [True, False])
def test_refined_shapes_on_both_kernels(gpu, monkeypatch, T, n, d, sym):
    """65 .. 128 refined cells (two bands): small launches take the band-parallel kernel of gram_band.hip, large ones the
    refined-grid kernel of gram_dyad.hip; SIGSVGD_BAND_MODE=serial keeps a small launch on gram_dyad.hip.  Both against the
    oracle, and reproducible."""
    from sigsvgd_amd import ops

    A, B = 11, 11 if sym else 7
    X = walks(A, T, d, 31, 0.2)
    Y = X if sym else walks(B, T, d, 32, 0.2)
    go = np.random.default_rng(4).uniform(0.5, 1.5, (A, B)).astype(np.float32)
    Kref, gref = C.gram_fwd_bwd(X, Y, 1.0, n, grad_out=go.astype(np.float64))
    Xg, gog = torch.as_tensor(X, device=gpu), torch.as_tensor(go, device=gpu)
    Yg = Xg if sym else torch.as_tensor(Y, device=gpu)
    res = {}
    for mode in ("serial", "parallel"):
        monkeypatch.setenv("SIGSVGD_BAND_MODE", mode)
        K, g = ops.gram_fwd_bwd(Xg, Yg, 1.0, n, grad_out=gog, y_is_x=sym)
        Kf = ops.gram_fwd(Xg, Yg, 1.0, n, y_is_x=sym)
        K2, g2 = ops.gram_fwd_bwd(Xg, Yg, 1.0, n, grad_out=gog, y_is_x=sym)
        torch.cuda.synchronize()
        assert torch.equal(K, K2) and torch.equal(g, g2)
        assert rel_entry(K.cpu().numpy(), Kref, 1e-6) < TOL and rel_entry(Kf.cpu().numpy(), Kref, 1e-6) < TOL
        assert rel_max(g.cpu().numpy(), gref) < TOL
        res[mode] = K.cpu().numpy()
    assert rel_entry(res["parallel"], res["serial"].astype(np.float64), 1e-6) < TOL
