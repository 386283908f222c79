"""The Matern-3/2 and -5/2 static kernels (SIGSVGD_STATIC_MATERN32 / _MATERN52) on every route that
evaluates a static kernel in fp64: the long-path solver's modes (csrc/gram_long.hip, csrc/pair_bands.hip), the coverage kernel
(csrc/gram_generic.hip), the bandwidth launches and the public surface on top of them, against the numpy reference of
tests/matern_reference.py (tests/test_matern_cpu.py ties it to central differences).

Tolerances are those of tests/test_gpu_static_kinds.py and tests/test_gpu_long.py: K per entry below 1e-9 with fp64 I/O and
below 2^-23 with fp32 I/O (every reference here has min |K| >= 0.5, asserted by `rel_entry(..., min_ref=0.5)`), gradients and
dK/d(1/h) below 1e-5 of their largest entry, shares and schedules that must agree bit for bit by `torch.equal`.  Inputs are
`O.synthetic_inputs` with signed weights from a seeded generator and h = 1, as in that file.  Y = X cases put coincident points
on every diagonal cell: there the square root's argument is clamped at 0 and the gradient term is zero, not NaN."""
import functools
import os

import numpy as np
import pytest
import torch

import matern_reference as MR
from oracle import sigkernel_oracle as O
from parity import np64, rel_entry, rel_max

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
KINDS = list(MR.KINDS)
H = 1.0


def ktol(io):
    return 1e-9 if io == F64 else 2.0**-23  # (fp32 I/O: K within its one rounding to fp32)


@functools.lru_cache(maxsize=None)
def inputs(A, T, d, seed):
    """fp32 values (the library's fp32 I/O reads them unrounded), as fp64 numpy; callers leave them unchanged"""
    return O.synthetic_inputs(A, T, d, seed_x=seed)[0].double().numpy()


@functools.lru_cache(maxsize=None)
def weights(A, B, seed=11):
    return np.random.default_rng(seed).standard_normal((A, B))  # signed


@functools.lru_cache(maxsize=None)
def reference(A, B, TX, TY, d, n, kind, weighted=True, sym=False, yseed=5):
    """(K, gX, gY) of X = inputs(A, TX, d, 0), Y = inputs(B, TY, d, yseed) (yseed 0: Y = X), shared by the tests of a shape"""
    w = weights(A, B) if weighted else None
    return MR.gram_backward(inputs(A, TX, d, 0), inputs(B, TY, d, yseed), w, kind, H, n, sym=sym)


@functools.lru_cache(maxsize=None)
def reference_dk(A, B, TX, TY, d, n, kind, yseed=5):
    return MR.dK_dinvh(inputs(A, TX, d, 0), inputs(B, TY, d, yseed), kind, H, n)


def dev(a, gpu, io=F64):
    return torch.as_tensor(a, dtype=io, device=gpu)


def finite(*ts):
    return all(bool(torch.isfinite(t).all()) for t in ts)


# ---- 1. long route, ordered pairs --------------------------------------------------------------------------------------------
# (A, B, TX, TY, d, n, sym, io): two bands of rows, > 63 columns per fill pass and points per gradient pass, TX != TY; d > 16 (the
# general static_k and the second 16-channel chunk of the gradient pass), refined; P = 66, a two-row second band (sym, Y = X)
LONG_CASES = [(3, 4, 70, 66, 3, 0, False, F64), (2, 3, 9, 12, 17, 2, False, F64), (5, 5, 34, 34, 2, 1, True, F64),
              (3, 4, 70, 66, 3, 0, False, F32)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("A,B,TX,TY,d,n,sym,io", LONG_CASES)
def test_long_route_ordered_pairs(gpu, A, B, TX, TY, d, n, sym, io, kind):
    from sigsvgd_amd import ops

    yseed = 0 if sym else 5
    Kr, gr, _ = reference(A, B, TX, TY, d, n, kind, True, sym, yseed)
    X, Y, go = dev(inputs(A, TX, d, 0), gpu, io), dev(inputs(B, TY, d, yseed), gpu, io), dev(weights(A, B), gpu, io)
    K, gX = ops.gram_long_fwd_bwd(X, Y, 1.0 / H, n, kind, go, sym=sym)
    print("long", (A, B, TX, TY, d, n, sym, io, kind), rel_entry(np64(K), Kr, 0.0, min_ref=0.5), rel_max(np64(gX), gr))
    assert K.dtype == io and gX.dtype == io and gX.shape == X.shape and finite(K, gX)
    assert rel_entry(np64(K), Kr, 0.0, min_ref=0.5) < ktol(io)
    assert rel_max(np64(gX), gr) < 1e-5
    assert torch.equal(ops.gram_long_fwd(X, Y, 1.0 / H, n, kind), K)
    K2, g2 = ops.gram_long_fwd_bwd(X, Y, 1.0 / H, n, kind, go, sym=sym)
    assert torch.equal(K, K2) and torch.equal(gX, g2)


# ---- 2. two-sided ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("io", [F64, F32])
def test_two_sided_both_slots(gpu, kind, io):
    from sigsvgd_amd import ops

    A, B, TX, TY, d, n = 3, 4, 70, 66, 3, 0
    Kr, gxr, gyr = reference(A, B, TX, TY, d, n, kind)
    X, Y, go = dev(inputs(A, TX, d, 0), gpu, io), dev(inputs(B, TY, d, 5), gpu, io), dev(weights(A, B), gpu, io)
    K, gX, gY = ops.gram_long_fwd_bwd2(X, Y, 1.0 / H, n, kind, go)
    print("long2", kind, io, rel_entry(np64(K), Kr, 0.0, min_ref=0.5), rel_max(np64(gX), gxr), rel_max(np64(gY), gyr))
    assert rel_entry(np64(K), Kr, 0.0, min_ref=0.5) < ktol(io)
    assert rel_max(np64(gX), gxr) < 1e-5 and rel_max(np64(gY), gyr) < 1e-5
    assert torch.equal(K, ops.gram_long_fwd(X, Y, 1.0 / H, n, kind))
    K2, gX2, gY2 = ops.gram_long_fwd_bwd2(X, Y, 1.0 / H, n, kind, go)
    assert torch.equal(K, K2) and torch.equal(gX, gX2) and torch.equal(gY, gY2)


@pytest.mark.parametrize("kind", KINDS)
def test_two_sided_y_is_x(gpu, kind):
    """Each unordered pair once: K mirrored bit for bit and gX the first-slot gradient, as the ordered launch returns it;
    coincident points on every diagonal cell of every pair (i, i)."""
    from sigsvgd_amd import ops

    A, T, d, n = 5, 34, 2, 1
    Kr, gxr, _ = reference(A, A, T, T, d, n, kind, yseed=0)
    X, go = dev(inputs(A, T, d, 0), gpu), dev(weights(A, A), gpu)
    K, gX, gY = ops.gram_long_fwd_bwd2(X, X, 1.0 / H, n, kind, go, y_is_x=True)
    assert gY is None and torch.equal(K, K.T) and finite(K, gX)
    print("long2 yx", kind, rel_entry(np64(K), Kr, 0.0, min_ref=0.5), rel_max(np64(gX), gxr))
    assert rel_entry(np64(K), Kr, 0.0, min_ref=0.5) < 1e-9 and rel_max(np64(gX), gxr) < 1e-5
    Ko, go_ = ops.gram_long_fwd_bwd(X, X, 1.0 / H, n, kind, go)
    assert rel_entry(np64(K), np64(Ko), 0.0, min_ref=0.5) < 1e-9 and rel_max(np64(gX), np64(go_)) < 1e-5


# ---- 3. paired ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("A,TX,TY,d,n,io", [(5, 70, 66, 3, 0, F64), (4, 9, 12, 17, 2, F64), (5, 70, 66, 3, 0, F32)])
def test_paired(gpu, A, TX, TY, d, n, io, kind):
    from sigsvgd_amd import ops

    Xn, Yn, w = inputs(A, TX, d, 0), inputs(A, TY, d, 5), weights(A, A)[0]
    Kr, gxr, gyr = MR.pair_backward(Xn, Yn, w, kind, H, n)
    X, Y = dev(Xn, gpu, io), dev(Yn, gpu, io)
    K, gX, gY = ops.pair_fwd_bwd(X, Y, 1.0 / H, n, kind, dev(w, gpu, io))
    print("pair", (A, TX, TY, d, n, io, kind), rel_entry(np64(K), Kr, 0.0, min_ref=0.5), rel_max(np64(gX), gxr), rel_max(np64(gY), gyr))
    assert rel_entry(np64(K), Kr, 0.0, min_ref=0.5) < ktol(io)
    assert rel_max(np64(gX), gxr) < 1e-5 and rel_max(np64(gY), gyr) < 1e-5
    assert torch.equal(K, ops.gram_long_fwd(X, Y, 1.0 / H, n, kind).diagonal())
    assert torch.equal(K, ops.pair_fwd(X, Y, 1.0 / H, n, kind))
    K2, gX2, gY2 = ops.pair_fwd_bwd(X, Y, 1.0 / H, n, kind, dev(w, gpu, io))
    assert torch.equal(K, K2) and torch.equal(gX, gX2) and torch.equal(gY, gY2)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("io", [F64, F32])
def test_band_schedule_matches_the_serial_one_bit_for_bit(gpu, monkeypatch, kind, io):
    """forced as tests/test_gpu_pair_bands.py forces it; five bands of rows, TX != TY"""
    from sigsvgd_amd import ops

    A, TX, TY, d, n = 3, 300, 130, 3, 0
    monkeypatch.setenv("SIGSVGD_PAIR_MODE", "bands")
    for want_grad in (True, False):
        assert ops.pair_schedule(A, TX, TY, d, n, kind, want_grad)[0] >= 2, "the band-parallel kernel does not take this shape"
    monkeypatch.setenv("SIGSVGD_PAIR_MODE", "serial")
    assert ops.pair_schedule(A, TX, TY, d, n, kind)[0] == 1
    X, Y, w = dev(inputs(A, TX, d, 0), gpu, io), dev(inputs(A, TY, d, 5), gpu, io), dev(weights(A, A)[0], gpu, io)
    out = {}
    for mode in ("serial", "bands"):
        monkeypatch.setenv("SIGSVGD_PAIR_MODE", mode)
        out[mode] = (ops.pair_fwd(X, Y, 1.0 / H, n, kind), *ops.pair_fwd_bwd(X, Y, 1.0 / H, n, kind, w))
    for s, b in zip(out["serial"], out["bands"]):
        assert torch.equal(s, b)
    assert torch.equal(out["bands"][0], out["bands"][1]) and finite(*out["bands"])
    if io == F64:
        Kr, gxr, gyr = MR.pair_backward(inputs(A, TX, d, 0), inputs(A, TY, d, 5), weights(A, A)[0], kind, H, n)
        _, K, gX, gY = out["bands"]
        assert rel_entry(np64(K), Kr, 0.0, min_ref=0.5) < 1e-9 and rel_max(np64(gX), gxr) < 1e-5 and rel_max(np64(gY), gyr) < 1e-5


# ---- 4. partial --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N,T,d,n,io", [(12, 70, 3, 0, F64), (10, 20, 2, 2, F64), (10, 20, 2, 2, F32)])
def test_partial_shares_add_up(gpu, N, T, d, n, io, kind):
    from sigsvgd_amd import ops

    Kr, gr, _ = reference(N, N, T, T, d, n, kind, yseed=0)
    X, go = dev(inputs(N, T, d, 0), gpu, io), dev(weights(N, N), gpu, io)
    Kf, gf, _ = ops.gram_long_fwd_bwd2(X, X, 1.0 / H, n, kind, go, y_is_x=True)
    assert rel_entry(np64(Kf), Kr, 0.0, min_ref=0.5) < ktol(io) and rel_max(np64(gf), gr) < 1e-5
    world = 2
    for fold in (True, False):
        Ks, gs = torch.zeros_like(Kf), torch.zeros(N, T, d, dtype=F64, device=gpu)
        for rank in range(world):
            Kp, gp = ops.gram_long_sym_partial(X, 1.0 / H, rank, world, n, kind, go, fold=fold)
            assert gp.dtype == F64
            Ks += Kp
            gs += gp
        assert torch.equal(Ks, Kf), fold  # (every pair is in one share: the sum adds zeros)
        print("partial", (N, T, d, n, io, kind, fold), rel_max(np64(gs), np64(gf)), rel_max(np64(gs), gr))
        if io == F64:
            assert rel_max(np64(gs), np64(gf)) < 1e-9
        assert rel_max(np64(gs), gr) < 1e-5


# ---- 5. coverage kernel ------------------------------------------------------------------------------------------------------
# (A, B, T, d, n, sym, io): 16 lanes share a row; 4 lanes share a row; two 16-channel chunks; two passes over the rows; sym;
# fp32 I/O
COVERAGE_CASES = [(5, 6, 4, 2, 3, False, F64), (5, 6, 10, 3, 2, False, F64), (5, 6, 20, 17, 0, False, F64),
                  (5, 6, 70, 3, 0, False, F64), (5, 5, 10, 3, 2, True, F64), (5, 6, 10, 3, 2, False, F32)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("A,B,T,d,n,sym,io", COVERAGE_CASES)
def test_coverage_kernel(gpu, A, B, T, d, n, sym, io, kind):
    """The default flags (what SigKernel launches) and force_generic, both at the tolerances of the module docstring"""
    from sigsvgd_amd import ops

    assert ops.gram_takes(A, B, T, d, n, kind, True, False, sym)
    Kr, gr, _ = reference(A, B, T, T, d, n, kind, True, sym)
    X, Y, go = dev(inputs(A, T, d, 0), gpu, io), dev(inputs(B, T, d, 5), gpu, io), dev(weights(A, B), gpu, io)
    for forced in (False, True):
        K, gX = ops.gram_fwd_bwd(X, Y, 1.0 / H, n, kind, go, sym=sym, force_generic=forced)
        K1 = ops.gram_fwd(X, Y, 1.0 / H, n, kind, force_generic=forced)
        eK, eK1 = rel_entry(np64(K), Kr, 0.0, min_ref=0.5), rel_entry(np64(K1), Kr, 0.0, min_ref=0.5)
        print("coverage", (A, B, T, d, n, sym, io, kind, forced), eK, eK1, rel_max(np64(gX), gr))
        assert finite(K, gX, K1) and eK < ktol(io) and eK1 < ktol(io)
        assert rel_max(np64(gX), gr) < 1e-5
        K2, g2 = ops.gram_fwd_bwd(X, Y, 1.0 / H, n, kind, go, sym=sym, force_generic=forced)
        assert torch.equal(K, K2) and torch.equal(gX, g2)
    if (T, n) == (10, 2) and not sym:  # the first-order solver is the coverage kernel's too
        Kn = ops.gram_fwd(X, Y, 1.0 / H, n, kind, naive=True)
        assert 1e-7 < rel_max(np64(Kn), Kr) < 1e-2  # (another stencil: close to, not equal to, the second-order solution)


@pytest.mark.parametrize("kind", KINDS)
def test_coverage_kernel_symmetric_solve(gpu, kind):
    """4,096 pairs with Y = X, each unordered pair solved once.  The kernel forms its distance as xn + yn - 2 dot, which for
    the coincident points of the pairs (i, i) rounds to either side of zero: without the clamp the square root gives NaN."""
    from sigsvgd_amd import ops

    N, T, d = 64, 6, 2
    Kr, gr, _ = reference(N, N, T, T, d, 0, kind, yseed=0)
    X, go = dev(inputs(N, T, d, 0), gpu), dev(weights(N, N), gpu)
    K, gX = ops.gram_fwd_bwd(X, X, 1.0 / H, 0, kind, go, y_is_x=True)
    print("coverage yx", kind, rel_entry(np64(K), Kr, 0.0, min_ref=0.5), rel_max(np64(gX), gr))
    assert finite(K, gX) and torch.equal(K, K.T)
    assert rel_entry(np64(K), Kr, 0.0, min_ref=0.5) < 1e-9 and rel_max(np64(gX), gr) < 1e-5


@pytest.mark.parametrize("kind", KINDS)
def test_coverage_kernel_and_long_route_agree(gpu, kind):
    from sigsvgd_amd import ops

    A, B, T, d, n = 5, 6, 60, 3, 1
    X, Y, go = dev(inputs(A, T, d, 0), gpu), dev(inputs(B, T, d, 5), gpu), dev(weights(A, B), gpu)
    assert ops.gram_takes(A, B, T, d, n, kind)
    Kl, gl = ops.gram_long_fwd_bwd(X, Y, 1.0 / H, n, kind, go)
    Kc, gc = ops.gram_fwd_bwd(X, Y, 1.0 / H, n, kind, go)
    print("overlap", kind, rel_entry(np64(Kc), np64(Kl), 0.0, min_ref=0.5), rel_max(np64(gc), np64(gl)))
    assert rel_entry(np64(Kc), np64(Kl), 0.0, min_ref=0.5) < 1e-9 and rel_max(np64(gc), np64(gl)) < 1e-5


# ---- 6. the bandwidth derivative ---------------------------------------------------------------------------------------------
def same(a, b):
    return (a is None and b is None) or torch.equal(a, b)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("A,B,TX,TY,d,n,yx", [(3, 4, 20, 17, 2, 0, False), (5, 5, 12, 12, 2, 1, True)])
def test_bandwidth_gram_launch(gpu, kind, A, B, TX, TY, d, n, yx):
    from sigsvgd_amd import ops

    yseed = 0 if yx else 5
    ref = reference_dk(A, B, TX, TY, d, n, kind, yseed)
    X, Y, go = dev(inputs(A, TX, d, 0), gpu), dev(inputs(B, TY, d, yseed), gpu), dev(weights(A, B), gpu)
    K, gX, gY, dK = ops.gram_long_fwd_bwd_h(X, Y, 1.0 / H, n, kind, go, y_is_x=yx)
    print("gram_h", kind, (A, B, TX, TY, d, n, yx), rel_max(np64(dK), ref))
    assert dK.shape == (A, B) and finite(dK) and rel_max(np64(dK), ref) < 1e-5
    K0, gX0, gY0 = ops.gram_long_fwd_bwd2(X, Y, 1.0 / H, n, kind, go, y_is_x=yx)
    assert torch.equal(K, K0) and same(gX, gX0) and same(gY, gY0) and gX is not None and (gY is None) == yx
    assert torch.equal(dK, ops.gram_long_fwd_bwd_h(X, Y, 1.0 / H, n, kind, go, y_is_x=yx)[3])
    if yx:
        assert torch.equal(dK, dK.T)


@pytest.mark.parametrize("kind", KINDS)
def test_bandwidth_paired_launch(gpu, kind):
    from sigsvgd_amd import ops

    A, TX, TY, d, n = 4, 10, 12, 2, 0
    Xn, Yn = inputs(A, TX, d, 0), inputs(A, TY, d, 5)
    ref = MR.pair_dK_dinvh(Xn, Yn, kind, H, n)
    X, Y, w = dev(Xn, gpu), dev(Yn, gpu), dev(weights(A, A)[0], gpu)
    K, gX, gY, dK = ops.pair_fwd_bwd_h(X, Y, 1.0 / H, n, kind, w)
    print("pair_h", kind, rel_max(np64(dK), ref))
    assert dK.shape == (A,) and rel_max(np64(dK), ref) < 1e-5
    K0, gX0, gY0 = ops.pair_fwd_bwd(X, Y, 1.0 / H, n, kind, w)
    assert torch.equal(K, K0) and torch.equal(gX, gX0) and torch.equal(gY, gY0)
    assert torch.equal(dK, ops.pair_fwd_bwd_h(X, Y, 1.0 / H, n, kind, w)[3])


# ---- 7. public surface -------------------------------------------------------------------------------------------------------
class Disguised:
    """a static kernel behind upstream's interface only: the library cannot recognise it (user route)"""

    def __init__(self, inner):
        self.Gram_matrix = inner.Gram_matrix
        self.batch_kernel = inner.batch_kernel


def _static(kind, sigma):
    import sigsvgd_amd.sigkernel as sk

    return sk.Matern32StaticKernel(sigma) if kind == MR.MATERN32 else sk.Matern52StaticKernel(sigma)


@pytest.mark.parametrize("T,n", [(20, 1), (300, 0)])  # the coverage kernel; the long route
def test_compute_gram(gpu, T, n):
    import sigsvgd_amd.sigkernel as sk
    from sigsvgd_amd import ops

    kind = MR.MATERN52
    A, B, d = 3, 4, 3
    assert ops.gram_takes(A, B, T, d, n, kind) == (T == 20)
    Kr1, gr1, _ = reference(A, B, T, T, d, n, kind, weighted=False)
    Kr, gr, gyr = reference(A, B, T, T, d, n, kind)
    Y, W = dev(inputs(B, T, d, 5), gpu), dev(weights(A, B), gpu)
    out = []
    for static in (_static(kind, H), Disguised(_static(kind, H))):
        k = sk.SigKernel(static, n)
        X = dev(inputs(A, T, d, 0), gpu).requires_grad_(True)
        K = k.compute_Gram(X, Y)
        K.sum().backward()  # unit grad_output
        g1 = X.grad.clone()
        X.grad = None
        (W * k.compute_Gram(X, Y)).sum().backward()  # signed grad_output
        out.append((np64(K), np64(g1), np64(X.grad)))
    (K, g1, gw), (Ku, g1u, gwu) = out
    eK, eKu = rel_entry(K, Kr, 0.0, min_ref=0.5), rel_entry(K, Ku, 0.0, min_ref=0.5)
    print("compute_Gram", T, n, eK, rel_max(g1, gr1), rel_max(gw, gr), eKu, rel_max(gw, gwu))
    assert eK < 1e-9 and rel_max(g1, gr1) < 1e-5 and rel_max(gw, gr) < 1e-5
    assert eKu < 1e-9 and rel_max(g1, g1u) < 1e-5 and rel_max(gw, gwu) < 1e-5  # the user route on the same kernel
    # grad_Y: the second slot
    k = sk.SigKernel(_static(kind, H), n)
    X, Yg = dev(inputs(A, T, d, 0), gpu).requires_grad_(True), Y.clone().requires_grad_(True)
    (W * k.compute_Gram(X, Yg, grad_Y=True)).sum().backward()
    assert rel_max(np64(X.grad), gr) < 1e-5 and rel_max(np64(Yg.grad), gyr) < 1e-5
    # sym (Y = X: coincident points), on the built-in and on the user route
    Krs, grs, _ = reference(A, A, T, T, d, n, kind, True, True, yseed=0)
    for static in (_static(kind, H), Disguised(_static(kind, H))):
        Xs = dev(inputs(A, T, d, 0), gpu).requires_grad_(True)
        Ks = sk.SigKernel(static, n).compute_Gram(Xs, Xs, sym=True)
        (dev(weights(A, A), gpu) * Ks).sum().backward()
        assert finite(Ks, Xs.grad)
        assert rel_entry(np64(Ks), Krs, 0.0, min_ref=0.5) < 1e-9 and rel_max(np64(Xs.grad), grs) < 1e-5


def test_compute_kernel_and_mmd(gpu):
    import sigsvgd_amd.sigkernel as sk

    kind = MR.MATERN52
    A, TX, TY, d, n = 5, 70, 66, 3, 0
    Xn, Yn = inputs(A, TX, d, 0), inputs(A, TY, d, 5)
    Kr, gxr, gyr = MR.pair_backward(Xn, Yn, None, kind, H, n)
    got = []
    for static in (_static(kind, H), Disguised(_static(kind, H))):
        X, Y = dev(Xn, gpu).requires_grad_(True), dev(Yn, gpu).requires_grad_(True)
        K = sk.SigKernel(static, n).compute_kernel(X, Y)
        K.sum().backward()
        assert rel_entry(np64(K), Kr, 0.0, min_ref=0.5) < 1e-9
        assert rel_max(np64(X.grad), gxr) < 1e-5 and rel_max(np64(Y.grad), gyr) < 1e-5
        got.append(np64(K))
    assert rel_entry(got[0], got[1], 0.0, min_ref=0.5) < 1e-9
    # mmd = mean K_XX + mean K_YY - 2 mean K_XY, every gradient through its own slot(s)
    T = 20
    Xn, Yn = inputs(4, T, d, 0), inputs(5, T, d, 5)
    Kxx, gxx, _ = MR.gram_backward(Xn, Xn, None, kind, H, n, sym=True)
    Kyy, gyy, _ = MR.gram_backward(Yn, Yn, None, kind, H, n, sym=True)
    Kxy, gxy, gyx = MR.gram_backward(Xn, Yn, None, kind, H, n)
    ref = Kxx.mean() + Kyy.mean() - 2.0 * Kxy.mean()
    for static in (_static(kind, H), Disguised(_static(kind, H))):
        X, Y = dev(Xn, gpu).requires_grad_(True), dev(Yn, gpu).requires_grad_(True)
        mmd = sk.SigKernel(static, n).compute_mmd(X, Y, grad_Y=True)
        mmd.backward()
        assert abs(float(mmd.detach()) - ref) < 1e-9 * max(1.0, abs(ref))
        assert rel_max(np64(X.grad), gxx / 16.0 - 2.0 * gxy / 20.0) < 1e-5
        assert rel_max(np64(Y.grad), gyy / 25.0 - 2.0 * gyx / 20.0) < 1e-5


@pytest.mark.parametrize("kind", KINDS)
def test_sigma_gradient_matches_the_user_route(gpu, kind):
    """fails without the feature; a sigma that requires grad through the bandwidth launch and through torch autograd on the
    user route, as tests/test_gpu_bandwidth_grad.py holds it for the other kinds"""
    import sigsvgd_amd.sigkernel as sk

    A, B, TX, TY, d, n, sigma0 = 3, 4, 20, 17, 3, 1, 1.3
    Xn, Yn, Wn = inputs(A, TX, d, 0), inputs(B, TY, d, 5), weights(A, B)
    X, Y, W = dev(Xn, gpu), dev(Yn, gpu), dev(Wn, gpu)
    grads = []
    for disguise in (False, True):
        sigma = torch.tensor(sigma0, dtype=F64, device=gpu, requires_grad=True)
        static = _static(kind, sigma)
        (W * sk.SigKernel(Disguised(static) if disguise else static, n).compute_Gram(X, Y)).sum().backward()
        grads.append(float(sigma.grad))
    ref = float(-(1.0 / sigma0) ** 2 * (Wn * MR.dK_dinvh(Xn, Yn, kind, sigma0, n)).sum())
    print("sigma grad", kind, grads, ref)
    assert abs(grads[0] - grads[1]) <= 1e-5 * abs(grads[1]) and abs(grads[0] - ref) <= 1e-5 * abs(ref)


@pytest.mark.parametrize("kind", KINDS)
def test_median_bandwidth_and_svgd_step(gpu, kind):
    import sigsvgd_amd.sigkernel as sk
    from sigsvgd_amd.inference import SVGD
    from sigsvgd_amd.kernels import BatchMatern32Kernel, BatchMatern52Kernel, SignatureKernel

    N, T, d = 8, 20, 3
    Xs, score = O.synthetic_inputs(N, T, d)
    Xn = Xs.double().numpy()
    cls = BatchMatern32Kernel if kind == MR.MATERN32 else BatchMatern52Kernel
    h = O.bw_median(MR.sqdist(Xn, Xn))
    Xg = Xs.to(gpu)
    Km = SignatureKernel(depth=0, static_kernel=MR.NAMES[kind])(Xg.double(), Xg.double())  # the default median, on the device
    Kh = SignatureKernel(lambda _: h, depth=0, static_kernel=MR.NAMES[kind])(Xg.double(), Xg.double())
    Kr, gr, _ = MR.gram_backward(Xn, Xn, None, kind, h, 0)
    print("median", kind, h, rel_entry(np64(Km), np64(Kh), 0.0, min_ref=0.5), rel_entry(np64(Km), Kr, 0.0, min_ref=0.5))
    assert rel_entry(np64(Km), np64(Kh), 0.0, min_ref=0.5) < 1e-9 and rel_entry(np64(Km), Kr, 0.0, min_ref=0.5) < 1e-9
    # one SVGD step with the named static kernel against the reference's velocity
    kernel = SignatureKernel(lambda _: h, depth=0, static_kernel=MR.NAMES[kind])
    assert type(kernel.kernel.static_kernel) is cls
    Xnew, info = SVGD(kernel, optimizer_class=None, lr=0.05).step(Xg.clone(), score.to(gpu))
    v = O.svgd_velocity(Kr, score.numpy(), gr)
    print("svgd", kind, rel_max(np64(info["grad"]), v), rel_max(np64(Xnew), Xn - 0.05 * v))
    assert rel_max(np64(info["grad"]), v) < 1e-5 and rel_max(np64(Xnew), Xn - 0.05 * v) < 1e-5


def test_sharded_step(gpu):
    """One rank, kind 7: a coverage-kernel shape steps row-wise, T = 300 takes the long partial solve, and with
    long_partial=False the long route's ordered launch row-wise; every route matches the unsharded step."""
    import torch.distributed as dist

    from sigsvgd_amd import ops
    from sigsvgd_amd.distributed import ShardedSigSVGD

    kind = MR.MATERN52
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ["MASTER_PORT"] = str(29571 + kind)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=gpu)
    try:
        for (N, T, d, route, kw) in [(8, 20, 2, "rowwise", {}), (8, 300, 2, "long_partial", {}),
                                     (8, 300, 2, "rowwise", {"long_partial": False})]:
            X, s = O.synthetic_inputs(N, T, d)
            Xg, sg = X.to(gpu), s.to(gpu)
            sh = ShardedSigSVGD(1.0 / H, 1e-3, static_kind=kind, **kw)
            Xa = sh.step(Xg, sg)
            assert sh.last_route == route, (T, sh.last_route)
            if route == "long_partial":
                K, g, _ = ops.gram_long_fwd_bwd2(Xg, Xg, 1.0 / H, 0, kind, y_is_x=True)
                assert torch.equal(sh.gather_gram(), K)
            elif T == 300:
                K, g = ops.gram_long_fwd_bwd(Xg, Xg, 1.0 / H, 0, kind)
            else:
                K, g = ops.gram_fwd_bwd(Xg, Xg, 1.0 / H, 0, kind)
            _, Xb = ops.svgd_phi(K, sg, g, X=Xg, lr=1e-3)
            assert rel_max(np64(Xa), np64(Xb)) < 1e-6
            Kr, gr, _ = reference(N, N, T, T, d, 0, kind, weighted=False, yseed=0)  # (inputs(N, T, d, 0) is X)
            v = O.svgd_velocity(Kr, s.numpy(), gr)
            print("sharded", kind, T, route, rel_max(np64(Xa), X.double().numpy() - 1e-3 * v))
            assert rel_max(np64(Xa), X.double().numpy() - 1e-3 * v) < 1e-5
    finally:
        dist.destroy_process_group()
