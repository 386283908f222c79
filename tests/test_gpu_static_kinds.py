"""The IMQ and rational-quadratic static kernels (SIGSVGD_STATIC_IMQ / _RQ) on every route that
evaluates a static kernel in fp64: the long-path solver's four modes (csrc/gram_long.hip), the coverage kernel
(csrc/gram_generic.hip) and the public surface on top of them, against the numpy reference of tests/radial_reference.py.

Tolerances are those of tests/test_gpu_long.py and tests/test_gpu_long_partial.py: K per entry below 1e-9 with fp64 I/O and
below 2^-23 with fp32 I/O (every reference here has min |K| >= 0.5, asserted, so the plain per-entry metric has nothing small
under it), gradients below 1e-5 of their largest entry, shares against the full launch bit for bit in K and below 1e-9 in
the fp64 gradient."""
import functools
import os

import numpy as np
import pytest
import torch

import radial_reference as RR
from oracle import sigkernel_oracle as O
from parity import np64, rel_entry, rel_max

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
KINDS = [RR.IMQ, RR.RQ]
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
    return RR.gram_backward(inputs(A, TX, d, 0), inputs(B, TY, d, yseed), w, kind, H, n, sym=sym)


def dev(a, gpu, io=F64):
    return torch.as_tensor(a, dtype=io, device=gpu)


# ---- 1. long route, ordered pairs --------------------------------------------------------------------------------------------
# (A, B, TX, TY, d, n, sym): two bands of rows, > 63 columns per fill pass and points per gradient pass, TX != TY; d > 16 (the
# general static_k and the second 16-channel chunk of the gradient pass), refined; P = 66, a two-row second band (sym once)
LONG_CASES = [(3, 4, 70, 66, 3, 0, False, F64), (2, 3, 9, 12, 17, 2, False, F64), (5, 5, 34, 34, 2, 1, True, F64),
              (3, 4, 70, 66, 3, 0, False, F32)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("A,B,TX,TY,d,n,sym,io", LONG_CASES)
def test_long_route_ordered_pairs(gpu, A, B, TX, TY, d, n, sym, io, kind):
    from sigsvgd_amd import ops

    Kr, gr, _ = reference(A, B, TX, TY, d, n, kind, True, sym)
    X, Y, go = dev(inputs(A, TX, d, 0), gpu, io), dev(inputs(B, TY, d, 5), gpu, io), dev(weights(A, B), gpu, io)
    K, gX = ops.gram_long_fwd_bwd(X, Y, 1.0 / H, n, kind, go, sym=sym)
    print("long", (A, B, TX, TY, d, n, sym, io, kind), rel_entry(np64(K), Kr, 0.0, min_ref=0.5), rel_max(np64(gX), gr))
    assert K.dtype == io and gX.dtype == io and gX.shape == X.shape
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
    """Each unordered pair once: K mirrored bit for bit; gX is the first-slot gradient, and with sym (the weights
    symmetrised) the sum of both slots' gradients."""
    from sigsvgd_amd import ops

    A, T, d, n = 6, 34, 2, 1
    Kr, gxr, gyr = reference(A, A, T, T, d, n, kind, yseed=0)
    X, go = dev(inputs(A, T, d, 0), gpu), dev(weights(A, A), gpu)
    K, gX, gY = ops.gram_long_fwd_bwd2(X, X, 1.0 / H, n, kind, go, y_is_x=True)
    assert gY is None and torch.equal(K, K.T)
    print("long2 yx", kind, rel_entry(np64(K), Kr, 0.0, min_ref=0.5), rel_max(np64(gX), gxr))
    assert rel_entry(np64(K), Kr, 0.0, min_ref=0.5) < 1e-9 and rel_max(np64(gX), gxr) < 1e-5
    Ks, gs, _ = ops.gram_long_fwd_bwd2(X, X, 1.0 / H, n, kind, go, sym=True, y_is_x=True)
    assert torch.equal(Ks, K) and rel_max(np64(gs), gxr + gyr) < 1e-5


# ---- 3. paired ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("A,TX,TY,d,n,io", [(5, 70, 66, 3, 0, F64), (4, 9, 12, 17, 2, F64), (5, 70, 66, 3, 0, F32)])
def test_paired(gpu, A, TX, TY, d, n, io, kind):
    from sigsvgd_amd import ops

    Xn, Yn, w = inputs(A, TX, d, 0), inputs(A, TY, d, 5), weights(A, A)[0]
    Kr, gxr, gyr = RR.pair_backward(Xn, Yn, w, kind, H, n)
    X, Y = dev(Xn, gpu, io), dev(Yn, gpu, io)
    K, gX, gY = ops.pair_fwd_bwd(X, Y, 1.0 / H, n, kind, dev(w, gpu, io))
    print("pair", (A, TX, TY, d, n, io, kind), rel_entry(np64(K), Kr, 0.0, min_ref=0.5), rel_max(np64(gX), gxr), rel_max(np64(gY), gyr))
    assert rel_entry(np64(K), Kr, 0.0, min_ref=0.5) < ktol(io)
    assert rel_max(np64(gX), gxr) < 1e-5 and rel_max(np64(gY), gyr) < 1e-5
    assert torch.equal(K, ops.gram_long_fwd(X, Y, 1.0 / H, n, kind).diagonal())
    assert torch.equal(K, ops.pair_fwd(X, Y, 1.0 / H, n, kind))
    K2, gX2, gY2 = ops.pair_fwd_bwd(X, Y, 1.0 / H, n, kind, dev(w, gpu, io))
    assert torch.equal(K, K2) and torch.equal(gX, gX2) and torch.equal(gY, gY2)


# ---- 4. partial --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N,T,d,n,io", [(12, 70, 3, 0, F64), (10, 20, 2, 2, F64), (10, 20, 2, 2, F32)])
def test_partial_shares_add_up(gpu, N, T, d, n, io, kind):
    from sigsvgd_amd import ops

    Kr, gr, _ = reference(N, N, T, T, d, n, kind, yseed=0)
    X, go = dev(inputs(N, T, d, 0), gpu, io), dev(weights(N, N), gpu, io)
    Kf, gf, _ = ops.gram_long_fwd_bwd2(X, X, 1.0 / H, n, kind, go, y_is_x=True)
    assert rel_entry(np64(Kf), Kr, 0.0, min_ref=0.5) < ktol(io) and rel_max(np64(gf), gr) < 1e-5
    for world in (2, 3):
        for fold in (True, False):
            Ks, gs = torch.zeros_like(Kf), torch.zeros(N, T, d, dtype=F64, device=gpu)
            for rank in range(world):
                Kp, gp = ops.gram_long_sym_partial(X, 1.0 / H, rank, world, n, kind, go, fold=fold)
                assert gp.dtype == F64
                Kq, gq = ops.gram_long_sym_partial(X, 1.0 / H, rank, world, n, kind, go, fold=fold)
                assert torch.equal(Kp, Kq) and torch.equal(gp, gq)  # two launches, the same bits
                Ks += Kp
                gs += gp
            assert torch.equal(Ks, Kf), (world, fold)  # (every pair is in one share: the sum adds zeros)
            print("partial", (N, T, d, n, io, kind, world, fold), rel_max(np64(gs), np64(gf)), rel_max(np64(gs), gr))
            if io == F64:
                assert rel_max(np64(gs), np64(gf)) < 1e-9
            assert rel_max(np64(gs), gr) < 1e-5


# ---- 5. coverage kernel ------------------------------------------------------------------------------------------------------
# (A, B, T, d, n, sym, io): 16 lanes share a row; 4 lanes share a row; two 16-channel chunks; two passes over the rows; the
# long-path (`big`) layout of generic_plan (tests/test_gpu_longpaths.py: T = 128, d = 14 with the gradient); sym once
COVERAGE_CASES = [(5, 6, 4, 2, 3, False, F64), (5, 6, 10, 3, 2, False, F64), (5, 6, 20, 17, 0, False, F64),
                  (5, 6, 70, 3, 0, False, F64), (5, 6, 128, 14, 0, False, F64), (5, 5, 10, 3, 2, True, F64),
                  (5, 6, 10, 3, 2, False, F32)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("A,B,T,d,n,sym,io", COVERAGE_CASES)
def test_coverage_kernel(gpu, A, B, T, d, n, sym, io, kind):
    """The default flags (what SigKernel launches) and force_generic, both at the tolerances of the module docstring: the two
    kinds take the plan that keeps the increments in fp64."""
    from sigsvgd_amd import ops

    assert ops.gram_takes(A, B, T, d, n, kind, True, False, sym)
    Kr, gr, _ = reference(A, B, T, T, d, n, kind, True, sym)
    X, Y, go = dev(inputs(A, T, d, 0), gpu, io), dev(inputs(B, T, d, 5), gpu, io), dev(weights(A, B), gpu, io)
    for forced in (False, True):
        K, gX = ops.gram_fwd_bwd(X, Y, 1.0 / H, n, kind, go, sym=sym, force_generic=forced)
        K1 = ops.gram_fwd(X, Y, 1.0 / H, n, kind, force_generic=forced)
        eK, eK1 = rel_entry(np64(K), Kr, 0.0, min_ref=0.5), rel_entry(np64(K1), Kr, 0.0, min_ref=0.5)
        print("coverage", (A, B, T, d, n, sym, io, kind, forced), eK, eK1, rel_max(np64(gX), gr))
        assert eK < ktol(io) and eK1 < ktol(io)
        assert rel_max(np64(gX), gr) < 1e-5
        K2, g2 = ops.gram_fwd_bwd(X, Y, 1.0 / H, n, kind, go, sym=sym, force_generic=forced)
        assert torch.equal(K, K2) and torch.equal(gX, g2) and torch.equal(K1, ops.gram_fwd(X, Y, 1.0 / H, n, kind, force_generic=forced))
    if (T, n) == (10, 2) and not sym:  # the first-order solver is the coverage kernel's too
        Kn = ops.gram_fwd(X, Y, 1.0 / H, n, kind, naive=True)
        assert 1e-7 < rel_max(np64(Kn), Kr) < 1e-2  # (another stencil: close to, not equal to, the second-order solution)


@pytest.mark.parametrize("kind", KINDS)
def test_coverage_kernel_symmetric_solve(gpu, kind):
    """4,096 pairs with Y = X: each unordered pair is solved once, the column-side contraction runs, K is mirrored"""
    from sigsvgd_amd import ops

    N, T, d = 64, 6, 2
    Kr, gr, _ = reference(N, N, T, T, d, 0, kind, yseed=0)
    X, go = dev(inputs(N, T, d, 0), gpu), dev(weights(N, N), gpu)
    K, gX = ops.gram_fwd_bwd(X, X, 1.0 / H, 0, kind, go, y_is_x=True)
    print("coverage yx", kind, rel_entry(np64(K), Kr, 0.0, min_ref=0.5), rel_max(np64(gX), gr))
    assert torch.equal(K, K.T)
    assert rel_entry(np64(K), Kr, 0.0, min_ref=0.5) < 1e-9 and rel_max(np64(gX), gr) < 1e-5
    K2, g2 = ops.gram_fwd_bwd(X, X, 1.0 / H, 0, kind, go, y_is_x=True)
    assert torch.equal(K, K2) and torch.equal(gX, g2)


@pytest.mark.parametrize("kind", KINDS)
def test_coverage_kernel_and_long_route_agree(gpu, kind):
    from sigsvgd_amd import ops

    A, B, T, d, n = 5, 6, 60, 3, 1
    X, Y, go = dev(inputs(A, T, d, 0), gpu), dev(inputs(B, T, d, 5), gpu), dev(weights(A, B), gpu)
    assert ops.gram_takes(A, B, T, d, n, kind)
    Kl, gl = ops.gram_long_fwd_bwd(X, Y, 1.0 / H, n, kind, go)
    for forced in (False, True):
        Kc, gc = ops.gram_fwd_bwd(X, Y, 1.0 / H, n, kind, go, force_generic=forced)
        print("overlap", kind, forced, rel_entry(np64(Kc), np64(Kl), 0.0, min_ref=0.5), rel_max(np64(gc), np64(gl)))
        assert rel_entry(np64(Kc), np64(Kl), 0.0, min_ref=0.5) < 1e-9 and rel_max(np64(gc), np64(gl)) < 1e-5


# ---- 6. public surface -------------------------------------------------------------------------------------------------------
class Disguised:
    """a static kernel behind upstream's interface only: the library cannot recognise it (user route)"""

    def __init__(self, inner):
        self.Gram_matrix = inner.Gram_matrix


def _static(kind, sigma):
    import sigsvgd_amd.sigkernel as sk

    return sk.IMQStaticKernel(sigma) if kind == RR.IMQ else sk.RationalQuadraticKernel(sigma)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T,n", [(20, 1), (300, 0)])  # the coverage kernel; the long route
def test_compute_gram(gpu, kind, T, n):
    import sigsvgd_amd.sigkernel as sk
    from sigsvgd_amd import ops

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
        K.sum().backward()
        g1 = X.grad.clone()
        X.grad = None
        (W * k.compute_Gram(X, Y)).sum().backward()
        out.append((np64(K), np64(g1), np64(X.grad)))
    (K, g1, gw), (Ku, g1u, gwu) = out
    eK, eKu = rel_entry(K, Kr, 0.0, min_ref=0.5), rel_entry(K, Ku, 0.0, min_ref=0.5)
    print("compute_Gram", kind, T, n, eK, rel_max(g1, gr1), rel_max(gw, gr), eKu, rel_max(gw, gwu))
    assert eK < 1e-9 and rel_max(g1, gr1) < 1e-5 and rel_max(gw, gr) < 1e-5
    assert eKu < 1e-9 and rel_max(g1, g1u) < 1e-5 and rel_max(gw, gwu) < 1e-5  # the user route on the same kernel
    # grad_Y: the second slot
    k = sk.SigKernel(_static(kind, H), n)
    X, Yg = dev(inputs(A, T, d, 0), gpu).requires_grad_(True), Y.clone().requires_grad_(True)
    (W * k.compute_Gram(X, Yg, grad_Y=True)).sum().backward()
    assert rel_max(np64(X.grad), gr) < 1e-5 and rel_max(np64(Yg.grad), gyr) < 1e-5
    # sym and gram_and_grad
    Ks, gs = k.gram_and_grad(dev(inputs(A, T, d, 0), gpu), None, dev(weights(A, A), gpu), sym=True)
    Krs, grs, _ = reference(A, A, T, T, d, n, kind, True, True, yseed=0)
    assert rel_entry(np64(Ks), Krs, 0.0, min_ref=0.5) < 1e-9 and rel_max(np64(gs), grs) < 1e-5


@pytest.mark.parametrize("kind", KINDS)
def test_compute_kernel_and_mmd(gpu, kind):
    import sigsvgd_amd.sigkernel as sk

    A, TX, TY, d, n = 5, 70, 66, 3, 0
    k = sk.SigKernel(_static(kind, H), n)
    Xn, Yn = inputs(A, TX, d, 0), inputs(A, TY, d, 5)
    Kr, gxr, gyr = RR.pair_backward(Xn, Yn, None, kind, H, n)
    X, Y = dev(Xn, gpu).requires_grad_(True), dev(Yn, gpu).requires_grad_(True)
    K = k.compute_kernel(X, Y)
    K.sum().backward()
    assert rel_entry(np64(K), Kr, 0.0, min_ref=0.5) < 1e-9 and rel_max(np64(X.grad), gxr) < 1e-5 and rel_max(np64(Y.grad), gyr) < 1e-5
    # mmd = mean K_XX + mean K_YY - 2 mean K_XY, every gradient through its own slot(s)
    T = 20
    Xn, Yn = inputs(4, T, d, 0), inputs(5, T, d, 5)
    Kxx, gxx, _ = RR.gram_backward(Xn, Xn, None, kind, H, n, sym=True)
    Kyy, gyy, _ = RR.gram_backward(Yn, Yn, None, kind, H, n, sym=True)
    Kxy, gxy, gyx = RR.gram_backward(Xn, Yn, None, kind, H, n)
    X, Y = dev(Xn, gpu).requires_grad_(True), dev(Yn, gpu).requires_grad_(True)
    mmd = k.compute_mmd(X, Y, grad_Y=True)
    mmd.backward()
    ref = Kxx.mean() + Kyy.mean() - 2.0 * Kxy.mean()
    assert abs(float(mmd) - ref) < 1e-9 * max(1.0, abs(ref))
    assert rel_max(np64(X.grad), gxx / 16.0 - 2.0 * gxy / 20.0) < 1e-5
    assert rel_max(np64(Y.grad), gyy / 25.0 - 2.0 * gyx / 20.0) < 1e-5
    d0 = float(k.compute_distance(X.detach(), X.detach()))
    assert abs(d0) < 1e-12


@pytest.mark.parametrize("kind", KINDS)
def test_median_bandwidth_and_svgd_step(gpu, kind):
    import sigsvgd_amd.sigkernel as sk
    from sigsvgd_amd.inference import SVGD
    from sigsvgd_amd.kernels import BatchIMQKernel, BatchRationalQuadraticKernel, SignatureKernel

    N, T, d = 8, 20, 3
    Xs, score = O.synthetic_inputs(N, T, d)
    Xn = Xs.double().numpy()
    cls = BatchIMQKernel if kind == RR.IMQ else BatchRationalQuadraticKernel
    h = O.bw_median(RR.sqdist(Xn, Xn))
    Xg = Xs.to(gpu)
    Km = sk.SigKernel(cls(), 0).compute_Gram(Xg.double(), Xg.double())  # the default median, selected on the device
    Kh = sk.SigKernel(cls(lambda _: h), 0).compute_Gram(Xg.double(), Xg.double())
    Kr, gr, _ = RR.gram_backward(Xn, Xn, None, kind, h, 0)
    print("median", kind, h, rel_entry(np64(Km), np64(Kh), 0.0, min_ref=0.5), rel_entry(np64(Km), Kr, 0.0, min_ref=0.5))
    assert rel_entry(np64(Km), np64(Kh), 0.0, min_ref=0.5) < 1e-9 and rel_entry(np64(Km), Kr, 0.0, min_ref=0.5) < 1e-9
    # one SVGD step with the named static kernel against the reference's velocity
    kernel = SignatureKernel(lambda _: h, depth=0, static_kernel=RR.NAMES[kind])
    assert type(kernel.kernel.static_kernel) is cls
    Xnew, info = SVGD(kernel, optimizer_class=None, lr=0.05).step(Xg.clone(), score.to(gpu))
    v = O.svgd_velocity(Kr, score.numpy(), gr)
    print("svgd", kind, rel_max(np64(info["grad"]), v), rel_max(np64(Xnew), Xn - 0.05 * v))
    assert rel_max(np64(info["grad"]), v) < 1e-5 and rel_max(np64(Xnew), Xn - 0.05 * v) < 1e-5


@pytest.mark.parametrize("kind", KINDS)
def test_sharded_step(gpu, kind):
    """One rank: a coverage-kernel shape steps row-wise, T = 300 takes the long partial solve; both match the unsharded step,
    a row-wise step at T = 300 runs on ops.gram_long_fwd_bwd."""
    import torch.distributed as dist

    from sigsvgd_amd import ops
    from sigsvgd_amd.distributed import ShardedSigSVGD

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


# ---- 7. the motivating property ----------------------------------------------------------------------------------------------
def test_distant_bundles_repel_under_imq_and_not_under_rbf(gpu):
    """tests/test_radial_reference.py's property on the device: between two bundles 30 apart RBF's signature kernel is
    exactly 1 with an exactly zero gradient, IMQ's is not and matches the reference."""
    from sigsvgd_amd import ops

    Xn = RR.separated_bundles()
    h = O.bw_median(O.pairwise_sqdist(Xn, Xn))
    cross = np.zeros((8, 8))
    cross[:4, 4:] = cross[4:, :4] = 1.0
    X, go = dev(Xn, gpu), dev(cross, gpu)
    for launch in (lambda k: ops.gram_fwd_bwd(X, X, 1.0 / h, 0, k, go, force_generic=True),
                   lambda k: ops.gram_long_fwd_bwd(X, X, 1.0 / h, 0, k, go)):
        K, g = launch(RR.RBF)
        assert bool((K[:4, 4:] == 1.0).all()) and bool((K[4:, :4] == 1.0).all()) and bool((g == 0.0).all())
        for kind in KINDS:
            Kr, gr, _ = RR.gram_backward(Xn, Xn, cross, kind, h, 0)
            K, g = launch(kind)
            print("bundles", kind, rel_entry(np64(K), Kr, 0.0, min_ref=0.5), rel_max(np64(g), gr), np.abs(gr).max())
            assert rel_entry(np64(K), Kr, 0.0, min_ref=0.5) < 1e-9 and rel_max(np64(g), gr) < 1e-5
            assert bool((K[:4, 4:] != 1.0).all()) and float(g.abs().amax(dim=(1, 2)).min()) > 0.0
