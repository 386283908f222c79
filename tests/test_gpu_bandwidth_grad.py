"""The gradient of a static-kernel sigma on the device: the bandwidth launches of the long route
(`ops.gram_long_fwd_bwd_h`, `ops.pair_fwd_bwd_h`, csrc/gram_long.hip with long_static.h's `static_bw_pass`) and the autograd
nodes `sigsvgd_amd.sigkernel` builds on them, for RBF, IMQ and the rational quadratic kernel.

Reference: tests/bandwidth_reference.py, the GG contraction (R * -phi'(s) * s).sum / h on `radial_reference._solve`
(tests/test_bandwidth_grad_cpu.py ties it to the oracle).  Inputs are `O.synthetic_inputs`, fp32 values as fp64, at
h = 0.5, 1 and 4.  Tolerance: the gradient rule of the other files, below 1e-5 of the largest reference entry
(`parity.rel_max`) -- what fp32 storage of the forward solution and of S costs is 1e-8 to 1.1e-7 at these shapes.  K and the
coordinate gradients are compared bit for bit with the launches without the bandwidth output."""
import functools

import numpy as np
import pytest
import torch

import radial_reference as RR
from bandwidth_reference import dK_dh, dK_dinvh
from oracle import sigkernel_oracle as O
from parity import np64, rel_max
from plans import device_cus, long2_plan

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
KINDS = [RR.RBF, RR.IMQ, RR.RQ]
HS = [0.5, 1.0, 4.0]


@functools.lru_cache(maxsize=None)
def inputs(A, T, d, seed):
    """fp32 values (the library's fp32 I/O reads them unrounded), as fp64 numpy; callers leave them unchanged"""
    return O.synthetic_inputs(A, T, d, seed_x=seed)[0].double().numpy()


@functools.lru_cache(maxsize=None)
def weights(A, B, seed=11):
    return np.random.default_rng(seed).standard_normal((A, B))  # signed


@functools.lru_cache(maxsize=None)
def reference(A, B, TX, TY, d, n, kind, h, yseed=5, naive=False):
    """dK/d(1/h) [A, B] of X = inputs(A, TX, d, 0), Y = inputs(B, TY, d, yseed) (yseed 0: Y = X); shared, left unchanged"""
    return dK_dinvh(inputs(A, TX, d, 0), inputs(B, TY, d, yseed), kind, h, n, naive)


def dev(a, gpu, io=F64):
    return torch.as_tensor(a, dtype=io, device=gpu)


def same(a, b):
    return (a is None and b is None) or torch.equal(a, b)


# ---- 1. the Gram launch ------------------------------------------------------------------------------------------------------
# (A, B, TX, TY, d, n, io): two row bands, more than 63 points per pass on both sides, TX != TY (both I/O types); d > 16,
# refined; one partial band and a pass with 3 live lanes
GRAM_CASES = [(3, 4, 70, 66, 3, 0, F64), (3, 4, 70, 66, 3, 0, F32), (2, 3, 9, 12, 17, 2, F64), (4, 4, 3, 5, 2, 0, F64)]


def check_gram(gpu, A, B, TX, TY, d, n, io, kind, yx=False, naive=False):
    from sigsvgd_amd import ops

    yseed = 0 if yx else 5
    X, Y, go = dev(inputs(A, TX, d, 0), gpu, io), dev(inputs(B, TY, d, yseed), gpu, io), dev(weights(A, B), gpu, io)
    for h in HS:
        ref = reference(A, B, TX, TY, d, n, kind, h, yseed, naive)
        K, gX, gY, dK = ops.gram_long_fwd_bwd_h(X, Y, 1.0 / h, n, kind, go, naive, y_is_x=yx)
        print("gram_h", (A, B, TX, TY, d, n, io, kind, yx, naive, h), rel_max(np64(dK), ref), np.abs(ref).max())
        assert dK.dtype == io and dK.shape == (A, B)
        assert rel_max(np64(dK), ref) < 1e-5
        K0, gX0, gY0 = ops.gram_long_fwd_bwd2(X, Y, 1.0 / h, n, kind, go, naive, y_is_x=yx)
        assert torch.equal(K, K0) and same(gX, gX0) and same(gY, gY0) and gX is not None and (gY is None) == yx
        K2, gX2, gY2, dK2 = ops.gram_long_fwd_bwd_h(X, Y, 1.0 / h, n, kind, go, naive, y_is_x=yx)
        assert torch.equal(K, K2) and same(gX, gX2) and same(gY, gY2) and torch.equal(dK, dK2)
        if yx:
            assert torch.equal(dK, dK.T)
    return dK


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("A,B,TX,TY,d,n,io", GRAM_CASES)
def test_gram_launch(gpu, A, B, TX, TY, d, n, io, kind):
    check_gram(gpu, A, B, TX, TY, d, n, io, kind)


@pytest.mark.parametrize("kind", KINDS)
def test_gram_launch_y_is_x(gpu, kind):
    """each unordered pair once: exactly symmetric, and both triangles match the reference (check_gram compares all of it)"""
    check_gram(gpu, 5, 5, 34, 34, 2, 1, F64, kind, yx=True)


@pytest.mark.parametrize("kind", KINDS)
def test_gram_launch_tiles_of_several_pairs(gpu, kind):
    from sigsvgd_amd import ops

    A, B, TX, TY, d, n, h = 67, 70, 5, 6, 2, 0, 1.0
    pl = long2_plan(A, B, TX, TY, d, n, True, True, False, device_cus())
    assert pl["IC"] * pl["JC"] > 1 and pl["items"] > pl["grid"], pl
    X, Y, go = dev(inputs(A, TX, d, 0), gpu), dev(inputs(B, TY, d, 5), gpu), dev(weights(A, B), gpu)
    ref = reference(A, B, TX, TY, d, n, kind, h)
    K, gX, gY, dK = ops.gram_long_fwd_bwd_h(X, Y, 1.0 / h, n, kind, go)
    print("gram_h tiles", kind, pl["IC"], pl["JC"], rel_max(np64(dK), ref))
    assert rel_max(np64(dK), ref) < 1e-5
    K0, gX0, gY0 = ops.gram_long_fwd_bwd2(X, Y, 1.0 / h, n, kind, go)
    assert torch.equal(K, K0) and torch.equal(gX, gX0) and torch.equal(gY, gY0)
    assert torch.equal(dK, ops.gram_long_fwd_bwd_h(X, Y, 1.0 / h, n, kind, go)[3])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("yx", [False, True])
def test_gram_launch_sigma_only(gpu, kind, yx):
    """neither coordinate gradient: the reverse sweep still runs; the same dK_dinvh, bit for bit, as with them"""
    from sigsvgd_amd import ops

    A, B, TX, TY, d, n = (5, 5, 34, 34, 2, 1) if yx else (3, 4, 70, 66, 3, 0)
    X, Y = dev(inputs(A, TX, d, 0), gpu), dev(inputs(B, TY, d, 0 if yx else 5), gpu)
    for h in HS:
        ref = reference(A, B, TX, TY, d, n, kind, h, 0 if yx else 5)
        K, gX, gY, dK = ops.gram_long_fwd_bwd_h(X, Y, 1.0 / h, n, kind, None, y_is_x=yx, want_gradX=False, want_gradY=False)
        assert gX is None and gY is None and rel_max(np64(dK), ref) < 1e-5
        assert torch.equal(K, ops.gram_long_fwd_bwd2(X, Y, 1.0 / h, n, kind, y_is_x=yx, want_gradX=False, want_gradY=False)[0])
        assert torch.equal(dK, ops.gram_long_fwd_bwd_h(X, Y, 1.0 / h, n, kind, dev(weights(A, B), gpu), y_is_x=yx)[3])
        Kx, gx, none_y, dKx = ops.gram_long_fwd_bwd_h(X, Y, 1.0 / h, n, kind, None, want_gradY=False, y_is_x=yx)
        assert none_y is None and torch.equal(dKx, dK) and torch.equal(Kx, K)


def test_gram_launch_first_order_stencil(gpu):
    """RBF has the first-order stencil on this route; there the value is the derivative of K itself"""
    check_gram(gpu, 2, 3, 9, 12, 3, 0, F64, RR.RBF, naive=True)


# ---- 2. the paired launch ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("TX,TY,d,n", [(70, 66, 3, 0), (9, 12, 17, 2)])
def test_paired_launch(gpu, TX, TY, d, n, kind):
    from sigsvgd_amd import ops

    A = 5
    X, Y, w = dev(inputs(A, TX, d, 0), gpu), dev(inputs(A, TY, d, 5), gpu), dev(weights(A, A)[0], gpu)
    for h in HS:
        ref = np.diagonal(reference(A, A, TX, TY, d, n, kind, h))
        K, gX, gY, dK = ops.pair_fwd_bwd_h(X, Y, 1.0 / h, n, kind, w)
        print("pair_h", (TX, TY, d, n, kind, h), rel_max(np64(dK), ref))
        assert dK.shape == (A,) and rel_max(np64(dK), ref) < 1e-5
        K0, gX0, gY0 = ops.pair_fwd_bwd(X, Y, 1.0 / h, n, kind, w)
        assert torch.equal(K, K0) and torch.equal(gX, gX0) and torch.equal(gY, gY0)
        assert torch.equal(dK, ops.gram_long_fwd_bwd_h(X, Y, 1.0 / h, n, kind)[3].diagonal())
        Ks, none_x, none_y, dKs = ops.pair_fwd_bwd_h(X, Y, 1.0 / h, n, kind, None, want_x=False, want_y=False)
        assert none_x is None and none_y is None and torch.equal(Ks, K) and torch.equal(dKs, dK)
    Xf, Yf = X.to(F32), Y.to(F32)
    K, gX, gY, dK = ops.pair_fwd_bwd_h(Xf, Yf, 1.0, n, kind, w.to(F32))
    K0, gX0, gY0 = ops.pair_fwd_bwd(Xf, Yf, 1.0, n, kind, w.to(F32))
    assert dK.dtype == F32 and rel_max(np64(dK), np.diagonal(reference(A, A, TX, TY, d, n, kind, 1.0))) < 1e-5
    assert torch.equal(K, K0) and torch.equal(gX, gX0) and torch.equal(gY, gY0)


# ---- 3. the public surface ---------------------------------------------------------------------------------------------------
SIGMA = 1.3
PUB = (3, 4, 20, 17, 3, 1)  # (A, B, TX, TY, d, n): a shape the fused kernels take


def static_of(kind, sigma):
    import sigsvgd_amd.sigkernel as sk

    return {RR.RBF: sk.RBFKernel, RR.IMQ: sk.IMQStaticKernel, RR.RQ: sk.RationalQuadraticKernel}[kind](sigma)


class Disguised:
    """a static kernel behind upstream's `Gram_matrix` only: the library cannot recognise it (user route, `ops.PDESolve`)"""

    def __init__(self, inner):
        self.Gram_matrix = inner.Gram_matrix


def learned(device="cpu"):
    return torch.tensor(SIGMA, dtype=F64, device=device, requires_grad=True)


def close(a, b):
    return abs(float(a) - float(b)) <= 1e-5 * abs(float(b))


@pytest.mark.parametrize("kind", KINDS)
def test_compute_gram_learns_sigma(gpu, kind):
    """fails without the feature: sigma.grad stays None"""
    import sigsvgd_amd.sigkernel as sk

    A, B, TX, TY, d, n = PUB
    Xn, Yn, Wn = inputs(A, TX, d, 0), inputs(B, TY, d, 5), weights(A, B)
    sigma = learned(gpu)
    X, Y, W = dev(Xn, gpu).requires_grad_(True), dev(Yn, gpu), dev(Wn, gpu)
    K = sk.SigKernel(static_of(kind, sigma), n).compute_Gram(X, Y)
    (W * K).sum().backward()
    ref = float((Wn * dK_dh(Xn, Yn, kind, SIGMA, n)).sum())
    Kr, gxr, _ = RR.gram_backward(Xn, Yn, Wn, kind, SIGMA, n)
    print("compute_Gram sigma", kind, float(sigma.grad), ref, rel_max(np64(X.grad), gxr))
    assert sigma.grad is not None and sigma.grad.shape == sigma.shape and sigma.grad.dtype == F64
    assert close(sigma.grad, ref)
    assert rel_max(np64(X.grad), gxr) < 1e-5 and rel_max(np64(K), Kr) < 1e-9
    # K.sum(): the speculated unit-weight gradients, and sigma's from the same saved derivative
    sigma.grad, X.grad = None, None
    sk.SigKernel(static_of(kind, sigma), n).compute_Gram(X, Y).sum().backward()
    assert close(sigma.grad, dK_dh(Xn, Yn, kind, SIGMA, n).sum())
    assert rel_max(np64(X.grad), RR.gram_backward(Xn, Yn, None, kind, SIGMA, n)[1]) < 1e-5


@pytest.mark.parametrize("kind", KINDS)
def test_compute_gram_matches_the_user_route(gpu, kind):
    """the same kernel as a user static kernel goes through `ops.PDESolve` and torch autograd: the same sigma.grad"""
    import sigsvgd_amd.sigkernel as sk

    A, B, TX, TY, d, n = PUB
    X, Y, W = dev(inputs(A, TX, d, 0), gpu), dev(inputs(B, TY, d, 5), gpu), dev(weights(A, B), gpu)
    grads = []
    for disguise in (False, True):
        sigma = learned(gpu)
        static = static_of(kind, sigma)
        (W * sk.SigKernel(Disguised(static) if disguise else static, n).compute_Gram(X, Y)).sum().backward()
        grads.append(float(sigma.grad))
    print("user route", kind, grads)
    assert close(grads[0], grads[1])


@pytest.mark.parametrize("kind", KINDS)
def test_compute_kernel_learns_sigma(gpu, kind):
    import sigsvgd_amd.sigkernel as sk

    A, _, TX, TY, d, n = PUB
    Xn, Yn, wn = inputs(A, TX, d, 0), inputs(A, TY, d, 5), weights(A, A)[0]
    sigma = learned(gpu)
    X, Y, w = dev(Xn, gpu).requires_grad_(True), dev(Yn, gpu).requires_grad_(True), dev(wn, gpu)
    k = sk.SigKernel(static_of(kind, sigma), n)
    (w * k.compute_kernel(X, Y)).sum().backward()
    ref = float((wn * np.diagonal(dK_dh(Xn, Yn, kind, SIGMA, n))).sum())
    _, gxr, gyr = RR.pair_backward(Xn, Yn, wn, kind, SIGMA, n)
    print("compute_kernel sigma", kind, float(sigma.grad), ref)
    assert close(sigma.grad, ref)
    assert rel_max(np64(X.grad), gxr) < 1e-5 and rel_max(np64(Y.grad), gyr) < 1e-5
    # compute_distance on three paired launches
    sigma.grad = None
    k.compute_distance(X.detach(), Y.detach()).backward()
    dxx, dyy = np.diagonal(dK_dh(Xn, Xn, kind, SIGMA, n)), np.diagonal(dK_dh(Yn, Yn, kind, SIGMA, n))
    dxy = np.diagonal(dK_dh(Xn, Yn, kind, SIGMA, n))
    assert close(sigma.grad, dxx.mean() + dyy.mean() - 2.0 * dxy.mean())


@pytest.mark.parametrize("kind", KINDS)
def test_compute_mmd_learns_sigma(gpu, kind):
    """three Grams: sym=True twice (K is unweighted by sym, so sigma's gradient is not doubled), and the cross term"""
    import sigsvgd_amd.sigkernel as sk

    T, d, n = 20, 3, 1
    Xn, Yn = inputs(4, T, d, 0), inputs(5, T, d, 5)
    sigma = learned(gpu)
    X, Y = dev(Xn, gpu).requires_grad_(True), dev(Yn, gpu).requires_grad_(True)
    sk.SigKernel(static_of(kind, sigma), n).compute_mmd(X, Y).backward()
    ref = dK_dh(Xn, Xn, kind, SIGMA, n).mean() + dK_dh(Yn, Yn, kind, SIGMA, n).mean() - 2.0 * dK_dh(Xn, Yn, kind, SIGMA, n).mean()
    _, gxx, _ = RR.gram_backward(Xn, Xn, None, kind, SIGMA, n, sym=True)
    _, gxy, _ = RR.gram_backward(Xn, Yn, None, kind, SIGMA, n)
    print("compute_mmd sigma", kind, float(sigma.grad), ref)
    assert close(sigma.grad, ref)
    assert rel_max(np64(X.grad), gxx / 16.0 - 2.0 * gxy / 20.0) < 1e-5


@pytest.mark.parametrize("kind", KINDS)
def test_sigma_on_the_cpu(gpu, kind):
    import sigsvgd_amd.sigkernel as sk

    A, B, TX, TY, d, n = PUB
    Xn, Yn, Wn = inputs(A, TX, d, 0), inputs(B, TY, d, 5), weights(A, B)
    sigma = torch.tensor([SIGMA], dtype=F32, requires_grad=True)  # one element, its own shape, dtype and device
    K = sk.SigKernel(static_of(kind, sigma), n).compute_Gram(dev(Xn, gpu), dev(Yn, gpu))
    (dev(Wn, gpu) * K).sum().backward()
    h = float(sigma.detach())
    assert sigma.grad.device.type == "cpu" and sigma.grad.shape == (1,) and sigma.grad.dtype == F32
    assert close(sigma.grad, (Wn * dK_dh(Xn, Yn, kind, h, n)).sum())


@pytest.mark.parametrize("kind", KINDS)
def test_other_sigmas_keep_their_route_and_bits(gpu, kind):
    """a float, a plain tensor and a no_grad block at the same inputs: K of today's launch, bit for bit"""
    import sigsvgd_amd.sigkernel as sk
    from sigsvgd_amd import ops

    A, B, TX, TY, d, n = PUB
    X, Y = dev(inputs(A, TX, d, 0), gpu), dev(inputs(B, TY, d, 5), gpu)
    assert ops.gram_takes(A, B, max(TX, TY), d, n, kind, False)
    K0 = ops.gram_fwd(X, Y, 1.0 / SIGMA, n, kind)
    assert torch.equal(sk.SigKernel(static_of(kind, SIGMA), n).compute_Gram(X, Y), K0)
    assert torch.equal(sk.SigKernel(static_of(kind, torch.tensor(SIGMA, dtype=F64)), n).compute_Gram(X, Y), K0)
    with torch.no_grad():
        assert torch.equal(sk.SigKernel(static_of(kind, learned()), n).compute_Gram(X, Y), K0)
    Xg = X.clone().requires_grad_(True)
    K1, g1 = ops.gram_fwd_bwd(X, Y, 1.0 / SIGMA, n, kind)
    K = sk.SigKernel(static_of(kind, SIGMA), n).compute_Gram(Xg, Y)
    K.sum().backward()
    assert torch.equal(K, K1) and torch.equal(Xg.grad, g1)
