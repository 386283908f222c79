"""The IMQ and rational-quadratic static kernels on the register-resident fp32-sweep kernel (`fp32_sweeps=True`,
SIGSVGD_FLAG_FP32_SWEEPS; csrc/gram_fast_kernel.h RADIAL = 1, csrc/gram_fast_radial.hip) against the fp64
numpy reference of tests/radial_reference.py, on inputs of `oracle.sigkernel_oracle.synthetic_inputs` with h = 1.

Tolerance: the fp32-sweep contract of include/sigsvgd_hip.h, K per entry `rel_entry(K, Kr, 0.0, min_ref=0.5) < 1e-5` and the
gradient `rel_max(g, gr) < 1e-5` of its largest entry.  On these inputs the reference has min |K| >= 0.81 (computed on the CPU;
min_ref asserts 0.5), so the plain per-entry metric has nothing small under it.  The tests print the worst error / tolerance
per case; profiles/fast_static.txt keeps a copy of one run (K at most 0.08 of the tolerance on the smooth inputs, 0.35 on the
rough ones; gradients at most 0.07 -- except the cross-bundle gradient of test_distant_bundles_repel_on_the_fp32_route, which
sits at 0.999 (IMQ) and 0.78 (rational quadratic) of it: there the terms of the contraction add up to 151 and 111 times the
largest gradient entry (computed on the CPU), and the contraction is fp32: 151 x 2^-24 = 9e-6).
Every shape sits at an edge of the kernel (the comments at the tables)."""
import functools
import os

import numpy as np
import pytest
import torch

import radial_reference as RR
from oracle import sigkernel_oracle as O
from parity import np64, rel_entry, rel_max, signed_weights, walks

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
KINDS = [RR.IMQ, RR.RQ]
H = 1.0
TOL = 1e-5


@functools.lru_cache(maxsize=None)
def inputs(A, T, d, seed):
    """fp32 values as fp64 numpy (the fp32 launches read them unrounded); callers leave them unchanged"""
    return O.synthetic_inputs(A, T, d, seed_x=seed)[0].double().numpy()


@functools.lru_cache(maxsize=None)
def weights(A, B):
    return signed_weights(A, B, 11)


@functools.lru_cache(maxsize=None)
def reference(A, B, T, d, kind, weighted=True, sym=False, yseed=5):
    """(K, gX, gY) of X = inputs(A, T, d, 0), Y = inputs(B, T, d, yseed) (yseed 0: Y = X); computed once per shape and kind"""
    w = weights(A, B) if weighted else None
    return RR.gram_backward(inputs(A, T, d, 0), inputs(B, T, d, yseed), w, kind, H, 0, sym=sym)


def dev(a, gpu, io=F64):
    return torch.as_tensor(a, dtype=io, device=gpu)


def report(what, case, eK, eg=None):
    print(f"fast_static {what} {case}: K {eK:.2e} ({eK / TOL:.3f} tol)" + ("" if eg is None else f" grad {eg:.2e} ({eg / TOL:.3f} tol)"))


# (A, B, T, d): smallest grid, 32-slot ring, two rows per wavefront, a partial second tile | ring 32, 4-channel layout with
# the norm in the padded channel | full 32-slot ring, 4 channels without padding, three tiles | ring 32, 8-channel LP | first
# shape of the 64-slot ring, 8-wave workgroups | P = 63, the sweep's second round (the RBF launch would take the fixed-window
# twin) | no LP | 16-channel layout, 4-wave workgroups (two shapes)
ORDERED = [(9, 5, 3, 2), (9, 5, 17, 3), (17, 6, 32, 4), (9, 7, 32, 7), (9, 7, 33, 5), (9, 7, 64, 7), (9, 7, 64, 8), (5, 6, 64, 9),
           (5, 6, 50, 16)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("io", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("A,B,T,d", ORDERED)
def test_ordered_launches(gpu, A, B, T, d, io, kind):
    """forward-only and gradient launches with signed weights; two identical launches give the same bits; the flagged K is not
    the default route's (fp64 I/O: the coverage kernel's K differs from an fp32 sweep's somewhere)"""
    from sigsvgd_amd import ops

    Kr, gr, _ = reference(A, B, T, d, kind)
    X, Y, go = dev(inputs(A, T, d, 0), gpu, io), dev(inputs(B, T, d, 5), gpu, io), dev(weights(A, B), gpu, io)
    K, gX = ops.gram_fwd_bwd(X, Y, 1.0 / H, 0, kind, go, fp32_sweeps=True)
    Kf = ops.gram_fwd(X, Y, 1.0 / H, 0, kind, fp32_sweeps=True)
    eK, eKf, eg = rel_entry(np64(K), Kr, 0.0, min_ref=0.5), rel_entry(np64(Kf), Kr, 0.0, min_ref=0.5), rel_max(np64(gX), gr)
    report("ordered", (A, B, T, d, str(io)[6:], RR.NAMES[kind]), max(eK, eKf), eg)
    assert K.dtype == io and gX.dtype == io and gX.shape == X.shape
    assert eK < TOL and eKf < TOL
    assert eg < TOL
    K2, g2 = ops.gram_fwd_bwd(X, Y, 1.0 / H, 0, kind, go, fp32_sweeps=True)
    assert torch.equal(K, K2) and torch.equal(gX, g2) and torch.equal(Kf, ops.gram_fwd(X, Y, 1.0 / H, 0, kind, fp32_sweeps=True))
    if io == F64:
        assert not torch.equal(K, ops.gram_fwd_bwd(X, Y, 1.0 / H, 0, kind, go)[0])
        assert not torch.equal(Kf, ops.gram_fwd(X, Y, 1.0 / H, 0, kind))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("io", [F64, F32], ids=["f64", "f32"])
def test_one_channel(gpu, io, kind):
    """forward only on the register-resident kernel; the gradient launch of one-channel paths stays on the coverage kernel, as
    for RBF: the flag changes none of its bits"""
    from sigsvgd_amd import ops

    A, B, T, d = 9, 5, 20, 1
    Kr, gr, _ = reference(A, B, T, d, kind)
    X, Y, go = dev(inputs(A, T, d, 0), gpu, io), dev(inputs(B, T, d, 5), gpu, io), dev(weights(A, B), gpu, io)
    Kf = ops.gram_fwd(X, Y, 1.0 / H, 0, kind, fp32_sweeps=True)
    eK = rel_entry(np64(Kf), Kr, 0.0, min_ref=0.5)
    report("one channel", (A, B, T, d, str(io)[6:], RR.NAMES[kind]), eK)
    assert eK < TOL and torch.equal(Kf, ops.gram_fwd(X, Y, 1.0 / H, 0, kind, fp32_sweeps=True))
    if io == F64:
        assert not torch.equal(Kf, ops.gram_fwd(X, Y, 1.0 / H, 0, kind))
    K, g = ops.gram_fwd_bwd(X, Y, 1.0 / H, 0, kind, go, fp32_sweeps=True)
    Kd, gd = ops.gram_fwd_bwd(X, Y, 1.0 / H, 0, kind, go)
    assert torch.equal(K, Kd) and torch.equal(g, gd) and rel_max(np64(g), gr) < TOL


# Y = X: (17, 17, 64, 7) three tiles of 8 rows, LP; the two larger ones have more items than resident workgroups, so a workgroup
# takes several items, on each ring: 136 x 8 x 2 has 17 tiles of 8 rows (two per wavefront) and 1,224 items for the 768
# workgroups the 32-slot ring keeps resident on 256 compute units; 72 x 33 x 2 has 9 tiles of 8 rows and 360 items for 256
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("io", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("N,T,d", [(17, 64, 7), (136, 8, 2), (72, 33, 2)])
def test_y_is_x(gpu, N, T, d, io, kind):
    """each unordered pair once: K mirrored bit for bit; the gradient against the reference's first slot, and with sym against
    gX + gY; forward only too.  At N = 136 the ordered gradient launch (18,496 pairs, 2,312 items) runs as well."""
    from sigsvgd_amd import ops

    Kr, gxr, gyr = reference(N, N, T, d, kind, yseed=0)
    X, go = dev(inputs(N, T, d, 0), gpu, io), dev(weights(N, N), gpu, io)
    K, gX = ops.gram_fwd_bwd(X, X, 1.0 / H, 0, kind, go, y_is_x=True, fp32_sweeps=True)
    Ks, gs = ops.gram_fwd_bwd(X, X, 1.0 / H, 0, kind, go, sym=True, y_is_x=True, fp32_sweeps=True)
    Kf = ops.gram_fwd(X, X, 1.0 / H, 0, kind, y_is_x=True, fp32_sweeps=True)
    eK, eg, egs = rel_entry(np64(K), Kr, 0.0, min_ref=0.5), rel_max(np64(gX), gxr), rel_max(np64(gs), gxr + gyr)
    report("y_is_x", (N, T, d, str(io)[6:], RR.NAMES[kind]), max(eK, rel_entry(np64(Kf), Kr, 0.0, min_ref=0.5)), max(eg, egs))
    assert torch.equal(K, K.T) and torch.equal(Kf, Kf.T) and torch.equal(Ks, K)
    assert eK < TOL and rel_entry(np64(Kf), Kr, 0.0, min_ref=0.5) < TOL
    assert eg < TOL and egs < TOL
    K2, g2 = ops.gram_fwd_bwd(X, X, 1.0 / H, 0, kind, go, y_is_x=True, fp32_sweeps=True)
    assert torch.equal(K, K2) and torch.equal(gX, g2)
    if io == F64:
        assert not torch.equal(K, ops.gram_fwd_bwd(X, X, 1.0 / H, 0, kind, go, y_is_x=True)[0])
    if N == 136:
        Ko, go_ = ops.gram_fwd_bwd(X, X.clone(), 1.0 / H, 0, kind, go, fp32_sweeps=True)
        eKo, ego = rel_entry(np64(Ko), Kr, 0.0, min_ref=0.5), rel_max(np64(go_), gxr)
        report("ordered, many items", (N, T, d, str(io)[6:], RR.NAMES[kind]), eKo, ego)
        assert eKo < TOL and ego < TOL


# ---- rough paths in one to three channels: the cancellation / conditioning flags and the fp64 repair pass for these kinds ------
def rough_reference(X, Y, kind, h):
    """K only, fp64: the static kernel from per-channel differences (no [A, B, T, T, d] array), the oracle's increments, and the
    oracle's second-order sweep (`O.pde_sweep`'s statement) with the pairs as the contiguous axis -- 7,056 pairs of 64 points
    in about two seconds.  test_rough_reference_is_the_radial_reference ties it to tests/radial_reference.py."""
    X, Y = X.astype(np.float64), Y.astype(np.float64)
    A, B, T = len(X), len(Y), X.shape[1]
    s = np.zeros((A, B, T, T))
    for c in range(X.shape[2]):
        dlt = X[:, None, :, None, c] - Y[None, :, None, :, c]
        s += dlt * dlt
    g = np.ascontiguousarray(np.moveaxis(O.increments(RR.phi(kind, s / float(h))).reshape(A * B, T - 1, T - 1), 0, -1))
    K = np.ones((T, T, A * B))
    for sig in range(2 * T - 3):
        p = np.arange(max(0, sig - T + 2), min(T - 1, sig + 1))
        q = sig - p
        gg = g[p, q]
        g2 = gg * gg / 12.0
        K[p + 1, q + 1] = (K[p + 1, q] + K[p, q + 1]) * (1.0 + 0.5 * gg + g2) - K[p, q] * (1.0 - g2)
    return K[-1, -1].reshape(A, B)


def test_rough_reference_is_the_radial_reference():
    for kind in KINDS:
        X, Y = walks(5, 9, 3, 1, 0.2), walks(4, 9, 3, 2, 0.2)
        assert np.abs(rough_reference(X, Y, kind, 0.1) - RR.gram(X.astype(np.float64), Y.astype(np.float64), kind, 0.1, 0)).max() < 1e-13


# tests/test_gpu_precision.py's SOAK_REGIMES at the register-resident kernel's lengths, and its one-channel sweep rows (forward
# only: the one-channel gradient launch is the coverage kernel's): same generator (parity.walks), seeds, scales and bandwidths
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("A,B,T,d,h,scale", [(36, 36, 32, 3, 0.1, 0.1), (84, 84, 64, 2, 0.1, 0.2)])
def test_rough_few_channel_regimes(gpu, A, B, T, d, h, scale, seed, kind):
    from sigsvgd_amd import ops

    X, Y = walks(A, T, d, 100 * T + 10 * d + seed, scale), walks(B, T, d, 100 * T + 10 * d + seed + 5, scale)
    Kr = rough_reference(X, Y, kind, h)
    Xg, Yg = torch.as_tensor(X, device=gpu), torch.as_tensor(Y, device=gpu)
    K, g = ops.gram_fwd_bwd(Xg, Yg, 1.0 / h, 0, kind, fp32_sweeps=True)
    Kf = ops.gram_fwd(Xg, Yg, 1.0 / h, 0, kind, fp32_sweeps=True)
    eK, eKf = rel_entry(np64(K), Kr, 1e-6), rel_entry(np64(Kf), Kr, 1e-6)
    report("rough", (A, B, T, d, h, scale, seed, RR.NAMES[kind]), max(eK, eKf))
    assert eK < TOL and eKf < TOL and bool(torch.isfinite(g).all())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N,T", [(12, 64), (12, 32)])
def test_rough_one_channel_rows(gpu, N, T, kind):
    from sigsvgd_amd import ops

    worst = 0.0
    for scale in (0.1, 0.2, 0.5):
        X = walks(N, T, 1, 0, scale)
        Xg = torch.as_tensor(X, device=gpu)
        for h in (0.02, 0.1, 0.5, 1.0):
            Kr = rough_reference(X, X, kind, h)
            for yx in (True, False):
                Kf = ops.gram_fwd(Xg, Xg if yx else Xg.clone(), 1.0 / h, 0, kind, y_is_x=yx, fp32_sweeps=True)
                e = rel_entry(np64(Kf), Kr, 1e-6)
                worst = max(worst, e)
                assert e < TOL, (scale, h, yx, e)
    report("rough one channel", (N, T, RR.NAMES[kind]), worst)


# ---- the symmetric partial solve -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N,T,d", [(17, 64, 7), (17, 20, 3)])
def test_partial_shares_add_up(gpu, N, T, d, kind):
    from sigsvgd_amd import ops

    Kr, gr, _ = reference(N, N, T, d, kind, yseed=0)
    X, go = dev(inputs(N, T, d, 0), gpu), dev(weights(N, N), gpu)
    Kf, gf = ops.gram_fwd_bwd(X, X, 1.0 / H, 0, kind, go, y_is_x=True, fp32_sweeps=True)
    with pytest.raises(RuntimeError, match="FP32_SWEEPS"):
        ops.gram_sym_partial(X, 1.0 / H, 0, 1, kind, go)
    for world in (1, 2, 3):
        for fold in (True, False):
            Ks, gs = torch.zeros_like(Kf), torch.zeros(N, T, d, dtype=F64, device=gpu)
            for rank in range(world):
                Kp, gp = ops.gram_sym_partial(X, 1.0 / H, rank, world, kind, go, fold=fold, fp32_sweeps=True)
                assert gp.dtype == F64
                Ks += Kp
                gs += gp
            assert torch.equal(Ks, Kf), (world, fold)  # (every pair is in one share: the sum adds zeros)
            e = rel_max(np64(gs), np64(gf))
            report("partial", (N, T, d, RR.NAMES[kind], world, fold), rel_entry(np64(Ks), Kr, 0.0, min_ref=0.5), rel_max(np64(gs), gr))
            assert e < 1e-9, (world, fold, e)
            assert rel_max(np64(gs), gr) < TOL


# ---- exactly sized, offset, poisoned workspaces ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_guarded_workspace(gpu, monkeypatch, kind):
    """a symmetric gradient launch (row segments and the column slab) and an ordered few-channel one (the flag area of the fp64
    pass, row segments) on a workspace of exactly the queried bytes, 255 B into its 256-B alignment, every byte 0xFF, between
    guards: the bits of the ordinary launch, no byte outside the plan"""
    from guarded_workspace import GuardedWorkspace
    from sigsvgd_amd import ops

    Xs, gos = dev(inputs(17, 64, 7, 0), gpu, F32), dev(weights(17, 17), gpu, F32)
    Xo, Yo, goo = dev(inputs(9, 17, 3, 0), gpu, F32), dev(inputs(5, 17, 3, 5), gpu, F32), dev(weights(9, 5), gpu, F32)
    launches = [lambda: ops.gram_fwd_bwd(Xs, Xs, 1.0 / H, 0, kind, gos, y_is_x=True, fp32_sweeps=True),
                lambda: ops.gram_fwd_bwd(Xo, Yo, 1.0 / H, 0, kind, goo, fp32_sweeps=True)]
    plain = [f() for f in launches]
    torch.cuda.synchronize()
    for fill, offset in (("ones", 1), ("random", 0)):
        with monkeypatch.context() as m:
            ws = GuardedWorkspace(fill, offset).install(m)
            for f, (K0, g0) in zip(launches, plain):
                K, g = f()
                ws.check()
                assert torch.equal(K, K0) and torch.equal(g, g0), (fill, offset)
            assert ws.count == 2 and min(ws.sizes) > 256


# ---- public surface -------------------------------------------------------------------------------------------------------------
def test_sigkernel_autograd(gpu):
    import sigsvgd_amd.sigkernel as sk

    A, B, T, d = 9, 7, 33, 5
    Kr1, gr1, _ = reference(A, B, T, d, RR.IMQ, weighted=False)
    Kr, gr, gyr = reference(A, B, T, d, RR.IMQ)
    k = sk.SigKernel(sk.IMQStaticKernel(H), 0, fp32_sweeps=True)
    X, Y, W = dev(inputs(A, T, d, 0), gpu).requires_grad_(True), dev(inputs(B, T, d, 5), gpu).requires_grad_(True), dev(weights(A, B), gpu)
    K = k.compute_Gram(X, Y)
    K.sum().backward()
    g1 = X.grad.clone()
    X.grad = None
    (W * k.compute_Gram(X, Y, grad_Y=True)).sum().backward()
    report("compute_Gram", (A, B, T, d), rel_entry(np64(K), Kr, 0.0, min_ref=0.5), max(rel_max(g1, gr1), rel_max(X.grad, gr), rel_max(Y.grad, gyr)))
    assert rel_entry(np64(K), Kr, 0.0, min_ref=0.5) < TOL and rel_max(g1, gr1) < TOL
    assert rel_max(X.grad, gr) < TOL and rel_max(Y.grad, gyr) < TOL
    Kd = sk.SigKernel(sk.IMQStaticKernel(H), 0).compute_Gram(X.detach(), Y.detach())
    assert not torch.equal(K.detach(), Kd) and rel_entry(np64(Kd), Kr, 0.0, min_ref=0.5) < 1e-9  # the default stays fp64


def test_signature_kernel_by_name(gpu):
    from sigsvgd_amd.kernels import SignatureKernel

    N, T, d = 17, 64, 7
    Kr, gr, _ = reference(N, N, T, d, RR.RQ, weighted=False, yseed=0)
    kernel = SignatureKernel(lambda _: H, depth=0, static_kernel="rq", fp32_sweeps=True)
    X = dev(inputs(N, T, d, 0), gpu, F32)
    K, gk = kernel.gram_and_grad(X)
    report("SignatureKernel rq", (N, T, d), rel_entry(np64(K), Kr, 0.0, min_ref=0.5), rel_max(gk, gr))
    assert rel_entry(np64(K), Kr, 0.0, min_ref=0.5) < TOL and rel_max(gk, gr) < TOL
    Kd, _ = SignatureKernel(lambda _: H, depth=0, static_kernel="rq").gram_and_grad(X.double())
    assert not torch.equal(K.double(), Kd)


def test_distant_bundles_repel_on_the_fp32_route(gpu):
    """tests/test_radial_reference.py's property on the new route: between two bundles 30 apart (median bandwidth) the cross
    entries of K are not 1, every path has a non-zero gradient, and both match the reference"""
    from sigsvgd_amd import ops

    Xn = RR.separated_bundles()
    h = O.bw_median(O.pairwise_sqdist(Xn, Xn))
    cross = np.zeros((8, 8))
    cross[:4, 4:] = cross[4:, :4] = 1.0
    X, go = dev(Xn, gpu), dev(cross, gpu)
    for kind in KINDS:
        Kr, gr, _ = RR.gram_backward(Xn, Xn, cross, kind, h, 0)
        for yx in (True, False):
            K, g = ops.gram_fwd_bwd(X, X if yx else X.clone(), 1.0 / h, 0, kind, go, y_is_x=yx, fp32_sweeps=True)
            report("bundles", (RR.NAMES[kind], yx), rel_entry(np64(K), Kr, 0.0, min_ref=0.5), rel_max(np64(g), gr))
            assert rel_entry(np64(K), Kr, 0.0, min_ref=0.5) < TOL and rel_max(np64(g), gr) < TOL
            # K != 1 between the bundles.  This route returns K at fp32 resolution (the sweeps resolve 1.5e-7 of it, kernel
            # header), and the reference's cross entries are 1 + O(1e-6) (IMQ: up to 8e-6, rational quadratic: up to 5e-7), so
            # an entry within a few fp32 ulps of 1 may come out as 1.0 exactly: every entry the reference puts at least 1e-6
            # (8 ulps) away from 1 must differ from 1, IMQ has such entries, and no kind may return all ones as RBF does.
            far = torch.as_tensor(np.abs(Kr - 1.0) >= 1e-6, device=gpu)
            far[:4, :4] = far[4:, 4:] = False
            assert bool((K[far] != 1.0).all()) and (kind != RR.IMQ or int(far.sum()) >= 8)
            assert bool((K[:4, 4:] != 1.0).any()) and bool((K[4:, :4] != 1.0).any())
            assert float(g.abs().amax(dim=(1, 2)).min()) > 0.0


def test_sharded_step_takes_the_partial_solve(gpu):
    import torch.distributed as dist

    from sigsvgd_amd import _lib, ops
    from sigsvgd_amd.distributed import ShardedSigSVGD

    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ["MASTER_PORT"] = "29583"
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=gpu)
    try:
        N, T, d = 24, 64, 7
        X, s = O.synthetic_inputs(N, T, d)
        Xg, sg = X.to(gpu), s.to(gpu)
        sh = ShardedSigSVGD(1.0 / H, 1e-2, static_kind=_lib.STATIC_IMQ, fp32_sweeps=True)
        assert sh.route(Xg) == "partial"
        assert ShardedSigSVGD(1.0 / H, 1e-2, static_kind=_lib.STATIC_IMQ).route(Xg) == "rowwise"
        Xa = sh.step(Xg, sg)
        assert sh.last_route == "partial"
        K, g = ops.gram_fwd_bwd(Xg, Xg, 1.0 / H, 0, _lib.STATIC_IMQ, y_is_x=True, fp32_sweeps=True)
        v, Xb = ops.svgd_phi(K, sg, g, X=Xg, lr=1e-2)
        assert torch.equal(sh.gather_gram(), K)
        assert rel_max(sh.last_v_rows, np64(v).reshape(N, T, d)) < 1e-6 and rel_max(Xa, np64(Xb)) < 1e-6
        Kr, gr, _ = reference(N, N, T, d, RR.IMQ, weighted=False, yseed=0)
        assert rel_max(Xa, X.double().numpy() - 1e-2 * O.svgd_velocity(Kr, s.numpy(), gr)) < TOL
        # the row-wise step of the same object passes the flag too: the register-resident kernel's K, not the coverage kernel's
        rw = ShardedSigSVGD(1.0 / H, 1e-2, static_kind=_lib.STATIC_IMQ, fp32_sweeps=True, rowwise=True)
        Xc = rw.step(Xg, sg)
        assert rw.last_route == "rowwise" and rel_max(Xc, np64(Xb)) < 1e-6
        assert torch.equal(rw.last_K_rows, ops.gram_fwd_bwd(Xg, Xg.clone(), 1.0 / H, 0, _lib.STATIC_IMQ, fp32_sweeps=True)[0])
    finally:
        dist.destroy_process_group()


def test_graphed_iteration(gpu):
    from sigsvgd_amd import _lib, ops
    from sigsvgd_amd.graph import GraphedSigSVGD

    X0, s0 = O.synthetic_inputs(24, 33, 5)
    X0, s0 = X0.to(gpu), s0.to(gpu)
    g = GraphedSigSVGD(X0, inv_h=1.0 / H, lr=1e-2, static_kind=_lib.STATIC_IMQ, fp32_sweeps=True)
    g.score.copy_(s0)
    g.step()
    K, gk = ops.gram_fwd_bwd(X0, X0, 1.0 / H, 0, _lib.STATIC_IMQ, y_is_x=True, fp32_sweeps=True)
    _, Xe = ops.svgd_phi(K, s0, gk, X=X0, lr=1e-2)
    torch.cuda.synchronize()
    assert torch.equal(g.K, K) and torch.equal(g.grad_k, gk) and torch.equal(g.X, Xe)
    assert not torch.equal(K, ops.gram_fwd_bwd(X0, X0, 1.0 / H, 0, _lib.STATIC_IMQ, y_is_x=True)[0])
