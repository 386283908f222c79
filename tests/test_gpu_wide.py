"""RBF paths of 17 to 32 channels on the register-resident fp32-sweep kernel (`fp32_sweeps=True`, SIGSVGD_FLAG_FP32_SWEEPS;
csrc/gram_fast_kernel.h at DPAD = 32, csrc/gram_fast_wide.hip) against the C oracle, on the inputs
`parity.walks(A, T, d, seed, 0.05)` with h = 1 (tests/wide_plans.py: `inputs`, `reference`).

Tolerance: the fp32-sweep contract of include/sigsvgd_hip.h, K per entry `rel_entry(K, Kr, 1e-6) < 1e-5` and the gradient
`rel_max(g, gr) < 1e-5` of its largest entry.  On these inputs the oracle's K of two different batches lies between 0.93 and 2.4
(with Y = X the diagonal reaches 527 at T = 64, d = 32) and every row's largest gradient entry is at least 0.18 of the launch's
largest (computed on the CPU), and K of the first 16 channels alone or without the last channel is more than 1e-3 away
(tests/test_wide_cabi.py).  The tests print the worst error / tolerance per case (pytest -s).

Shapes: d = 17 (one channel past the 16-channel layout), 24, 31 (the instantiations without the padded channel) and 32 (no
padding); T = 3 (the smallest grid), 32, 33 and 64 (the sweep's second round); 5 x 6 and 9 x 7 paths: past one 4-row tile and
ragged against it; and 9 x 100 at T = 8, d = 17: 300 items for the 256 workgroups a 256-CU device holds, so a workgroup takes a
second item.  With fp64 I/O the flagged K differs from the default route's somewhere (the coverage kernel sweeps in fp64): on a
library without the feature the bit is ignored and those assertions fail."""
import os

import numpy as np
import pytest
import torch

from parity import np64, rel_entry, rel_max
from wide_plans import H, inputs, reference, weights, wide_geometry

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
TOL = 1e-5
DS, TS = [17, 24, 31, 32], [3, 32, 33, 64]
RBF = 0


def dev(a, gpu, io=F64):
    return torch.as_tensor(a, dtype=io, device=gpu)


def report(what, case, eK, eg=None):
    print(f"wide {what} {case}: K {eK:.2e} ({eK / TOL:.3f} tol)" + ("" if eg is None else f" grad {eg:.2e} ({eg / TOL:.3f} tol)"))


def eK_of(K, Kr):
    return rel_entry(np64(K), Kr, 1e-6)


@pytest.mark.parametrize("io", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("A,B", [(5, 6), (9, 7)])
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("d", DS)
def test_ordered_launches(gpu, d, T, A, B, io):
    """forward only, gradient with signed weights and with grad_out = NULL; two identical launches give the same bits"""
    from sigsvgd_amd import ops

    Kr, gr, _ = reference(A, B, T, d)
    g1r = reference(A, B, T, d, weighted=False)[1]
    X, Y, go = dev(inputs(A, T, d, 0), gpu, io), dev(inputs(B, T, d, 5), gpu, io), dev(weights(A, B), gpu, io)
    K, gX = ops.gram_fwd_bwd(X, Y, 1.0 / H, 0, RBF, go, fp32_sweeps=True)
    K1, g1 = ops.gram_fwd_bwd(X, Y, 1.0 / H, 0, RBF, fp32_sweeps=True)
    Kf = ops.gram_fwd(X, Y, 1.0 / H, 0, RBF, fp32_sweeps=True)
    eK, eKf, eg, eg1 = eK_of(K, Kr), eK_of(Kf, Kr), rel_max(np64(gX), gr), rel_max(np64(g1), g1r)
    report("ordered", (A, B, T, d, str(io)[6:]), max(eK, eKf), max(eg, eg1))
    assert K.dtype == io and gX.dtype == io and gX.shape == X.shape and Kf.shape == (A, B)
    assert eK < TOL and eKf < TOL and eK_of(K1, Kr) < TOL
    assert eg < TOL and eg1 < TOL
    K2, g2 = ops.gram_fwd_bwd(X, Y, 1.0 / H, 0, RBF, go, fp32_sweeps=True)
    assert torch.equal(K, K2) and torch.equal(gX, g2) and torch.equal(K1, K)
    assert torch.equal(Kf, ops.gram_fwd(X, Y, 1.0 / H, 0, RBF, fp32_sweeps=True))
    if io == F64:  # the flagged launch is not the default route's
        assert not torch.equal(K, ops.gram_fwd_bwd(X, Y, 1.0 / H, 0, RBF, go)[0])
        assert not torch.equal(Kf, ops.gram_fwd(X, Y, 1.0 / H, 0, RBF))


@pytest.mark.parametrize("io", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("N", [5, 9])
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("d", DS)
def test_y_is_x(gpu, d, T, N, io):
    """each unordered pair once: K mirrored bit for bit; the gradient against the oracle's first slot, and with sym against the
    sum of both slots; forward only too"""
    from sigsvgd_amd import ops

    Kr, gxr, gyr = reference(N, N, T, d, yseed=0)
    X, go = dev(inputs(N, T, d, 0), gpu, io), dev(weights(N, N), gpu, io)
    K, gX = ops.gram_fwd_bwd(X, X, 1.0 / H, 0, RBF, go, y_is_x=True, fp32_sweeps=True)
    Ks, gs = ops.gram_fwd_bwd(X, X, 1.0 / H, 0, RBF, go, sym=True, y_is_x=True, fp32_sweeps=True)
    Kf = ops.gram_fwd(X, X, 1.0 / H, 0, RBF, y_is_x=True, fp32_sweeps=True)
    eK, eKf, eg, egs = eK_of(K, Kr), eK_of(Kf, Kr), rel_max(np64(gX), gxr), rel_max(np64(gs), gxr + gyr)
    report("y_is_x", (N, T, d, str(io)[6:]), max(eK, eKf), max(eg, egs))
    assert torch.equal(K, K.T) and torch.equal(Kf, Kf.T) and torch.equal(Ks, K)
    assert eK < TOL and eKf < TOL
    assert eg < TOL and egs < TOL
    K2, g2 = ops.gram_fwd_bwd(X, X, 1.0 / H, 0, RBF, go, y_is_x=True, fp32_sweeps=True)
    Ks2, gs2 = ops.gram_fwd_bwd(X, X, 1.0 / H, 0, RBF, go, sym=True, y_is_x=True, fp32_sweeps=True)
    assert torch.equal(K, K2) and torch.equal(gX, g2) and torch.equal(gs, gs2)
    if io == F64:
        assert not torch.equal(K, ops.gram_fwd_bwd(X, X, 1.0 / H, 0, RBF, go, y_is_x=True)[0])


@pytest.mark.parametrize("io", [F64, F32], ids=["f64", "f32"])
def test_a_launch_past_the_resident_grid(gpu, io):
    """9 x 100 paths of 8 points in 17 channels: three tiles by 100 columns, more items than workgroups on a device of up to 299
    compute units, so workgroups take a second item and cross from a tile into the next"""
    from plans import device_cus
    from sigsvgd_amd import ops

    A, B, T, d = 9, 100, 8, 17
    g = wide_geometry(A, B, False, device_cus())
    assert g["items"] == 300 and g["items"] > g["grid"]
    Kr, gr, _ = reference(A, B, T, d)
    X, Y, go = dev(inputs(A, T, d, 0), gpu, io), dev(inputs(B, T, d, 5), gpu, io), dev(weights(A, B), gpu, io)
    K, gX = ops.gram_fwd_bwd(X, Y, 1.0 / H, 0, RBF, go, fp32_sweeps=True)
    Kf = ops.gram_fwd(X, Y, 1.0 / H, 0, RBF, fp32_sweeps=True)
    eK, eKf, eg = eK_of(K, Kr), eK_of(Kf, Kr), rel_max(np64(gX), gr)
    report("past the grid", (A, B, T, d, str(io)[6:]), max(eK, eKf), eg)
    assert eK < TOL and eKf < TOL and eg < TOL
    K2, g2 = ops.gram_fwd_bwd(X, Y, 1.0 / H, 0, RBF, go, fp32_sweeps=True)
    assert torch.equal(K, K2) and torch.equal(gX, g2)


def test_guarded_workspace(gpu, monkeypatch):
    """a symmetric gradient launch (row segments and the column slab) and an ordered one on a workspace of exactly the queried
    bytes, 255 B into its 256-B alignment, every byte 0xFF, between guards: the bits of the ordinary launch, no byte outside"""
    from guarded_workspace import GuardedWorkspace
    from sigsvgd_amd import ops

    Xs, gos = dev(inputs(9, 33, 31, 0), gpu, F32), dev(weights(9, 9), gpu, F32)
    Xo, Yo, goo = dev(inputs(9, 64, 17, 0), gpu, F32), dev(inputs(7, 64, 17, 5), gpu, F32), dev(weights(9, 7), gpu, F32)
    launches = [lambda: ops.gram_fwd_bwd(Xs, Xs, 1.0 / H, 0, RBF, gos, y_is_x=True, fp32_sweeps=True),
                lambda: ops.gram_fwd_bwd(Xo, Yo, 1.0 / H, 0, RBF, goo, fp32_sweeps=True)]
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


# ---- composition with SIGSVGD_FLAG_NORMALIZED_FUSED --------------------------------------------------------------------------------
@pytest.mark.parametrize("io", [F64, F32], ids=["f64", "f32"])
def test_normalised_kernel_around_the_wide_launch(gpu, io):
    """`normalized=True` on top of the flag at d = 17, T = 12, against `log_k_reference.normalized_gram_and_grads` at the bounds of
    tests/test_gpu_normalized_fused.py: K^ 1e-5 per entry (plus 3 * 2^-24 with fp32 I/O), the gradient 1e-5 (max|t1| + max|t2|) of
    its two terms on the reference"""
    import log_k_reference as R
    import normalized_fused_reference as NF
    from sigsvgd_amd import ops

    A, B, T, d = 5, 6, 12, 17
    X, Y, w = inputs(A, T, d, 0).astype(np.float64), inputs(B, T, d, 5).astype(np.float64), weights(A, B)
    w = w.astype(np.float32).astype(np.float64)
    Kh, g_ref, _ = R.normalized_gram_and_grads(X, Y, w, R.RBF, H, 0)
    t1, t2 = NF.terms(X, Y, w, R.RBF, H, 0, False, False)
    g_bound = 1e-5 * (np.abs(t1).max() + np.abs(t2).max())
    K, gX = ops.gram_fwd_bwd(dev(X, gpu, io), dev(Y, gpu, io), 1.0 / H, 0, RBF, dev(w, gpu, io), normalized=True, fp32_sweeps=True)
    Kf = ops.gram_fwd(dev(X, gpu, io), dev(Y, gpu, io), 1.0 / H, 0, RBF, normalized=True, fp32_sweeps=True)
    k_bound = 1e-5 + (3 * 2.0**-24 if io == F32 else 0.0)
    fk = float((np.abs(np64(K) - Kh) / np.abs(Kh)).max() / k_bound)
    fkf = float((np.abs(np64(Kf) - Kh) / np.abs(Kh)).max() / k_bound)
    fg = float(np.abs(np64(gX) - g_ref).max() / g_bound)
    print(f"wide normalised {(A, B, T, d, str(io)[6:])}: K^ {max(fk, fkf):.2e} of its bound, gradient {fg:.2e} of its bound "
          f"(terms / result: {max(np.abs(t1).max(), np.abs(t2).max()) / np.abs(g_ref).max():.2f})")
    assert fk <= 1.0 and fkf <= 1.0 and fg <= 1.0
    # the launch inside is the flagged one: K^ is K of the flagged launch between the diagonals of flagged launches
    Ku = ops.gram_fwd(dev(X, gpu, F64), dev(Y, gpu, F64), 1.0 / H, 0, RBF, normalized=True)
    Kw = ops.gram_fwd(dev(X, gpu, F64), dev(Y, gpu, F64), 1.0 / H, 0, RBF, normalized=True, fp32_sweeps=True)
    assert not torch.equal(Ku, Kw)


# ---- public surface at N = 9, T = 8, d = 17 --------------------------------------------------------------------------------------
N_, T_, D_ = 9, 8, 17


def test_sigkernel_autograd(gpu):
    import sigsvgd_amd.sigkernel as sk
    from sigsvgd_amd import ops

    Kr, gr, gyr = reference(N_, N_, T_, D_, yseed=0)
    k = sk.SigKernel(sk.RBFKernel(H), 0, fp32_sweeps=True)
    X, W = dev(inputs(N_, T_, D_, 0), gpu), dev(weights(N_, N_), gpu)
    Xg = X.clone().requires_grad_(True)
    K = k.compute_Gram(Xg, Xg, sym=True)
    (g,) = torch.autograd.grad((W * K).sum(), Xg)
    report("compute_Gram", (N_, T_, D_), eK_of(K.detach(), Kr), rel_max(g, gr + gyr))
    assert eK_of(K.detach(), Kr) < TOL and rel_max(g, gr + gyr) < TOL
    Ko, go = ops.gram_fwd_bwd(X, X, 1.0 / H, 0, RBF, W, sym=True, y_is_x=True, fp32_sweeps=True)
    assert torch.equal(K.detach(), Ko) and rel_max(go, gr + gyr) < TOL  # (the backward's launch is its own: g is held to the oracle)
    Kk, gk = k.gram_and_grad(X)
    K1, g1 = ops.gram_fwd_bwd(X, X, 1.0 / H, 0, RBF, y_is_x=True, fp32_sweeps=True)
    assert torch.equal(Kk, K1) and torch.equal(gk, g1)
    assert rel_max(gk, reference(N_, N_, T_, D_, weighted=False, yseed=0)[1]) < TOL
    Kd = sk.SigKernel(sk.RBFKernel(H), 0).compute_Gram(X, X, sym=True)
    assert not torch.equal(K.detach(), Kd) and eK_of(Kd, Kr) < 1e-9  # the default stays the coverage kernel's fp64


def test_one_svgd_step_by_name(gpu):
    """one `SVGD.step` through `kernels.SignatureKernel(..., fp32_sweeps=True)`: K is the flagged launch's, and the velocity
    -((K score - grad_k) / N) against the oracle's K and first-slot gradient.  Bound per entry, as
    tests/test_gpu_normalized_fused.py derives it: K's relative bound through the product with the score, the gradient's bound,
    and the fp32 rounding of the velocity launch's sums ((N + 2) 2^-24 of the absolute terms), all over N."""
    import sigsvgd_amd.sigkernel as sk
    from sigsvgd_amd import ops
    from sigsvgd_amd.inference import SVGD
    from sigsvgd_amd.kernels import SignatureKernel

    N, lr, eps = N_, 1e-2, 2.0**-24
    Kr, gr, _ = reference(N_, N_, T_, D_, weighted=False, yseed=0)
    Xn = inputs(N_, T_, D_, 0).astype(np.float64)
    score = np.random.default_rng(4).standard_normal(Xn.shape).astype(np.float32).astype(np.float64)
    S, G = score.reshape(N, -1), gr.reshape(N, -1)
    v_ref = -((Kr @ S - G) / N).reshape(Xn.shape)
    bound = ((TOL + 3 * eps) * (Kr @ np.abs(S)) + TOL * np.abs(G).max() + (N + 2) * eps * (Kr @ np.abs(S) + np.abs(G))) / N
    kernel = SignatureKernel(depth=0, static_kernel=sk.RBFKernel(H), fp32_sweeps=True)
    X = dev(Xn, gpu, F32)
    X1, info = SVGD(kernel, optimizer_class=None, lr=lr, iter_dict_device=None).step(X, grad_log_p=dev(score, gpu, F32))
    K, _ = ops.gram_fwd_bwd(X, X, 1.0 / H, 0, RBF, y_is_x=True, fp32_sweeps=True)
    assert torch.equal(info["k_xx"], K) and eK_of(K, Kr) < TOL
    frac = float((np.abs(np64(info["grad"]) - v_ref).reshape(N, -1) / bound).max())
    print(f"wide SVGD.step {(N_, T_, D_)}: velocity {frac:.2e} of its bound")
    assert frac <= 1.0
    assert float(np.abs(np64(X1) - (Xn - lr * v_ref)).max()) <= lr * bound.max() + 4 * eps * np.abs(Xn).max()


def test_graphed_iteration(gpu):
    from sigsvgd_amd import ops
    from sigsvgd_amd.graph import GraphedSigSVGD

    X0 = dev(inputs(N_, T_, D_, 0), gpu, F32)
    s0 = dev(np.random.default_rng(5).standard_normal(X0.shape), gpu, F32)
    g = GraphedSigSVGD(X0, inv_h=1.0 / H, lr=1e-2, fp32_sweeps=True)
    g.score.copy_(s0)
    g.step()
    K, gk = ops.gram_fwd_bwd(X0, X0, 1.0 / H, 0, RBF, y_is_x=True, fp32_sweeps=True)
    _, Xe = ops.svgd_phi(K, s0, gk, X=X0, lr=1e-2)
    torch.cuda.synchronize()
    assert torch.equal(g.K, K) and torch.equal(g.grad_k, gk) and torch.equal(g.X, Xe)
    assert eK_of(K, reference(N_, N_, T_, D_, yseed=0)[0]) < TOL


def test_sharded_row_wise_step(gpu):
    import torch.distributed as dist

    from sigsvgd_amd import ops
    from sigsvgd_amd.distributed import ShardedSigSVGD

    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ["MASTER_PORT"] = "29587"
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=gpu)
    try:
        X = dev(inputs(N_, T_, D_, 0), gpu, F32)
        s = dev(np.random.default_rng(6).standard_normal(X.shape), gpu, F32)
        sh = ShardedSigSVGD(1.0 / H, 1e-2, fp32_sweeps=True)
        assert sh.route(X) == "rowwise"  # the partial solve keeps refusing d > 16
        sh.step(X, s)
        assert sh.last_route == "rowwise"
        K = ops.gram_fwd_bwd(X, X.clone(), 1.0 / H, 0, RBF, fp32_sweeps=True)[0]
        assert torch.equal(sh.last_K_rows, K)
        assert eK_of(K, reference(N_, N_, T_, D_, yseed=0)[0]) < TOL
    finally:
        dist.destroy_process_group()
