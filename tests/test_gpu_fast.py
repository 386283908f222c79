"""GPU parity: register-resident fast kernels (n=0, T<=64, RBF) vs the fp64 oracle, via the C ABI."""
import numpy as np
import pytest
import torch

from oracle import c_oracle as C
from oracle import sigkernel_oracle as O
from parity import rel_entry, rel_max, walks

pytestmark = pytest.mark.gpu

TOL = 1e-5  # north_star tolerance (relative; gradients relative to max-abs)
# two fp32-sweep solves of one pair that differ in orientation (the symmetric launch solves (i, j), the ordered one also
# (j, i)) or launch geometry agree to a few ulps PER ENTRY; both are within TOL of the fp64 oracle
SELF = 4e-6


SHAPES = [
    # A, B, T, d
    (9, 11, 64, 7),   # headline path shape, ragged row tile / column chunk
    (8, 8, 64, 7),
    (17, 5, 32, 7),   # C2 path shape
    (10, 13, 64, 3),  # C3 path shape
    (6, 7, 20, 2),
    (5, 9, 3, 7),     # shortest supported path (T=3)
    (7, 6, 33, 14),   # d > 8 variant (6-wave workgroups)
    (3, 4, 50, 1),
]


@pytest.mark.parametrize("A,B,T,d", SHAPES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_fast_general_xy(gpu, A, B, T, d, dtype):
    """X != Y: ordered pairs, row-side gradient only, arbitrary grad_out."""
    from sigsvgd_amd import ops

    X, Y = walks(A, T, d, 1, 0.05), walks(B, T, d, 2, 0.05)
    h = 1.3
    go = np.random.default_rng(3).standard_normal((A, B)).astype(np.float32)
    Kref, gref = C.gram_fwd_bwd(X, Y, h, 0, grad_out=go.astype(np.float64))
    Xg, Yg, gog = (torch.as_tensor(t, device=gpu).to(dtype) for t in (X, Y, go))
    K1 = ops.gram_fwd(Xg, Yg, 1.0 / h)
    K2, g2 = ops.gram_fwd_bwd(Xg, Yg, 1.0 / h, grad_out=gog)
    torch.cuda.synchronize()
    assert rel_entry(K1.cpu().numpy(), Kref, 1e-6) < TOL
    assert rel_entry(K2.cpu().numpy(), Kref, 1e-6) < TOL
    assert rel_max(g2.cpu().numpy(), gref) < TOL
    # and it agrees with the generic kernel
    K3, g3 = ops.gram_fwd_bwd(Xg, Yg, 1.0 / h, grad_out=gog, force_generic=True)
    assert rel_max(g2.cpu().numpy(), g3.double().cpu().numpy()) < TOL


@pytest.mark.parametrize("N,T,d", [(19, 64, 7), (8, 64, 7), (33, 32, 7), (12, 64, 3), (16, 20, 2), (13, 40, 14)])
@pytest.mark.parametrize("weights", ["ones", "random", "sym"])
def test_fast_symmetric(gpu, N, T, d, weights):
    """Y is X: unordered pairs solved once, row- and column-side gradients."""
    from sigsvgd_amd import ops

    X = walks(N, T, d, 5, 0.05)
    h = 0.9
    go = None
    sym = False
    if weights != "ones":
        go = np.random.default_rng(7).standard_normal((N, N)).astype(np.float32)
    if weights == "sym":
        sym = True
    Kref, gref = O.gram_backward(X, X, None if go is None else go.astype(np.float64), O.RBF, h, 0, False, sym)
    Xg = torch.as_tensor(X, device=gpu)
    gog = None if go is None else torch.as_tensor(go, device=gpu)
    K, g = ops.gram_fwd_bwd(Xg, Xg, 1.0 / h, grad_out=gog, sym=sym, y_is_x=True)
    torch.cuda.synchronize()
    Kn = K.cpu().numpy()
    assert rel_entry(Kn, Kref, 1e-6) < TOL
    assert np.array_equal(Kn, Kn.T)  # mirrored entries are the same solve
    assert rel_max(g.cpu().numpy(), gref) < TOL


def test_fast_far_from_origin(gpu):
    """Per-pair centring: particles far from the origin keep full accuracy."""
    from sigsvgd_amd import ops

    X = walks(12, 64, 7, 11, 0.05, offset=100.0)
    Kref, gref = O.gram_backward(X, X, None, O.RBF, 1.0, 0)
    K, g = ops.gram_fwd_bwd(torch.as_tensor(X, device=gpu), torch.as_tensor(X, device=gpu), 1.0, y_is_x=True)
    assert rel_entry(K.cpu().numpy(), Kref, 1e-6) < TOL
    assert rel_max(g.cpu().numpy(), gref) < TOL


def test_fast_c4_rows(gpu):
    """Headline size N=1024,T=64,d=7 on the benchmark's synthetic particles: K rows and grad rows of a
    subsample against the C oracle (full oracle run would take ~30 s of 8 cores)."""
    from sigsvgd_amd import ops

    X, _ = O.synthetic_inputs(1024, 64, 7)
    Xg = X.to(gpu)
    K, g = ops.gram_fwd_bwd(Xg, Xg, 1.0, y_is_x=True)
    torch.cuda.synchronize()
    Kn, gn = K.cpu().numpy(), g.cpu().numpy()
    assert np.isfinite(Kn).all() and np.isfinite(gn).all()
    assert np.array_equal(Kn, Kn.T)
    for rows in [(0, 4), (511, 515), (1020, 1024)]:
        Kref, gref = C.gram_fwd_bwd(X.numpy(), X.numpy(), 1.0, 0, rows=rows)
        assert rel_entry(Kn[rows[0]:rows[1]], Kref, 1e-6) < TOL
        assert np.abs(gn[rows[0]:rows[1]] - gref).max() / np.abs(gref).max() < TOL


@pytest.mark.parametrize("A,B,T,d", [(1, 1, 64, 7), (1, 9, 17, 2), (9, 1, 64, 8), (11, 11, 3, 16), (23, 23, 64, 5)])
def test_fast_edge_shapes(gpu, A, B, T, d):
    """single rows/columns, ragged row tiles, exact-fit channel padding (d = 8, 16)"""
    from sigsvgd_amd import ops

    X, Y = walks(A, T, d, 21, 0.05), walks(B, T, d, 22, 0.05)
    Kref, gref = C.gram_fwd_bwd(X, Y, 0.8, 0)
    Xg, Yg = torch.as_tensor(X, device=gpu), torch.as_tensor(Y, device=gpu)
    K, g = ops.gram_fwd_bwd(Xg, Yg, 1 / 0.8)
    assert rel_entry(K.cpu().numpy(), Kref, 1e-6) < TOL and rel_max(g.cpu().numpy(), gref) < TOL
    if A == B:
        Kr, gr = C.gram_fwd_bwd(X, X, 0.8, 0)
        K2, g2 = ops.gram_fwd_bwd(Xg, Xg, 1 / 0.8, y_is_x=True)
        assert rel_entry(K2.cpu().numpy(), Kr, 1e-6) < TOL and rel_max(g2.cpu().numpy(), gr) < TOL


def test_fast_fp64_io_symmetric_and_noncontiguous(gpu):
    """fp64 particles (what the reference's callers hand to compute_Gram) through the symmetric path,
    and a non-contiguous view as input"""
    from sigsvgd_amd import ops

    Xbig = torch.as_tensor(walks(20, 64, 14, 31, 0.05), device=gpu).double()
    Xv = Xbig[:, :, ::2]  # [20, 64, 7] strided view
    assert not Xv.is_contiguous()
    Kref, gref = O.gram_backward(Xv.cpu().numpy(), Xv.cpu().numpy(), None, O.RBF, 1.0, 0)
    K, g = ops.gram_fwd_bwd(Xv, Xv, 1.0, y_is_x=True)
    assert K.dtype == torch.float64 and g.dtype == torch.float64
    assert rel_entry(K.cpu().numpy(), Kref, 1e-6) < SELF and rel_max(g.cpu().numpy(), gref) < TOL


def test_argument_errors(gpu):
    from sigsvgd_amd import ops

    x = torch.zeros(4, 10, 3, device=gpu)
    assert tuple(ops.gram_fwd(x, torch.zeros(4, 9, 3, device=gpu), 1.0).shape) == (4, 4)  # ragged lengths: padded (round 4)
    with pytest.raises(ValueError):
        ops.gram_fwd(x, torch.zeros(4, 9, 3, device=gpu), 1.0, y_is_x=True)   # ... but not declared the same batch
    with pytest.raises(ValueError):
        ops.gram_fwd(x, torch.zeros(4, 10, 2, device=gpu), 1.0)     # channel mismatch
    with pytest.raises(ValueError):
        ops.gram_fwd(x[:0], x, 1.0)                                  # empty batch
    with pytest.raises(ValueError):
        ops.gram_fwd(x[:, :1], x[:, :1], 1.0)                        # single-point paths
    with pytest.raises(ValueError):
        ops.gram_fwd_bwd(x, x, 1.0, grad_out=torch.zeros(3, 4, device=gpu))
    with pytest.raises(TypeError):
        ops.gram_fwd(x.half(), x.half(), 1.0)
    with pytest.raises(RuntimeError, match="inv_h"):
        ops.gram_fwd(x, x, -1.0)


@pytest.mark.parametrize("N,T,d", [(21, 64, 7), (9, 33, 3), (12, 128, 14), (7, 100, 5)])
def test_forward_only_symmetric_solve(gpu, N, T, d):
    """gram_fwd(X, X, y_is_x=True): each unordered pair once, K mirrored == the ordered forward launch"""
    from sigsvgd_amd import ops

    X = torch.as_tensor(walks(N, T, d, 31, 0.05), device=gpu)
    K1 = ops.gram_fwd(X, X, 1.0, y_is_x=True)
    K0 = ops.gram_fwd(X, X.clone(), 1.0)
    assert torch.equal(K1, K1.T)
    assert rel_entry(K1.cpu().numpy(), K0.double().cpu().numpy(), 1e-6) < SELF


@pytest.mark.parametrize("T,d,scale,h", [(64, 2, 0.1, 0.1), (64, 2, 0.2, 0.1), (64, 2, 0.5, 1.0), (64, 2, 0.05, 0.02),
                                         (32, 2, 0.2, 0.1), (48, 3, 0.3, 0.3)])
def test_fast_oscillating_solutions_per_entry(gpu, T, d, scale, h):
    """Rough paths in few channels against a narrow static kernel: the discrete solution oscillates (negative entries) and
    K[P][P] can be a small remainder of much larger values on the pair's grid; the fp32 sweeps alone lose up to 1.9e-5 per
    entry there.  Pairs with max |K_grid| > 4 max(|K|, 0.1) repeat the forward sweep in fp64 (gram_fast.hip,
    resweep_fwd_fp64): every entry is inside the tolerance, in every launch form."""
    from sigsvgd_amd import ops

    X = walks(12, T, d, 0, scale=scale)
    Kref, gref = C.gram_fwd_bwd(X, X, h, 0)
    assert Kref.min() < 0.5  # (the regime the test is about: solutions that cancel)
    Xg = torch.as_tensor(X, device=gpu)
    outs = [ops.gram_fwd_bwd(Xg, Xg, 1.0 / h, y_is_x=True), ops.gram_fwd_bwd(Xg, Xg.clone(), 1.0 / h)]
    fwd = [ops.gram_fwd(Xg, Xg, 1.0 / h, y_is_x=True), ops.gram_fwd(Xg, Xg.clone(), 1.0 / h)]
    torch.cuda.synchronize()
    for K, g in outs:
        assert rel_entry(K.cpu().numpy(), Kref, 1e-6) < 5e-6
        assert rel_max(g.cpu().numpy(), gref) < TOL
    for K in fwd:
        assert rel_entry(K.cpu().numpy(), Kref, 1e-6) < 5e-6
