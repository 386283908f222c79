"""GPU parity in the ill-conditioned regimes: rough paths in one to three channels on the DEFAULT dispatch.

Round 3's soak (6,000 random cases, scripts/dev/soak.py) left 9 cases beyond 1e-5, all of them rough paths (|step|^2 / h
between 0.1 and 0.4 per channel) in one to three channels: K[P][P] is ill-conditioned in the increments there, and the fp32
STORAGE of the increments limits it whatever the precision of the sweeps.  The kernels now measure the condition number per
pair and hand the pairs beyond it to the exact fp64 pass (gram_fast.hip, "conditioning").  The soak did not record its seed,
so the nine cases are restated here by their regime -- shape, channels, step scale, bandwidth, launch form -- with fixed seeds
of this file; the d = 1 block is the one-channel part of scripts/precision_sweep.py (profiles/r03_precision_sweep.md: worst
1.9e-5 at T = 100, scale 0.2, h 0.02).  Reference: the static kernel and the Gram matrix are fp64 whatever the input
(/root/reference/src/kernels/_traj_kernels.py:204-206), so the bar is 1e-5 per entry in every regime.
"""
import numpy as np
import pytest
import torch

from oracle import c_oracle as C
from parity import rel_entry, rel_max, walks

pytestmark = pytest.mark.gpu

TOL = 1e-5


# (A, B, T, d, h, scale, Y is X): the regimes of the nine soak cases of round 3 (gpurun_out/soak_r3m.log: 213, 492, 1118, 1995,
# 2383, 2441, 3027, 3526, 4339) -- 3027 is the coverage kernel with the gradient at T = 100 (test_exact_pass_long_paths)
SOAK_REGIMES = [
    (19, 19, 100, 1, 1.0, 0.5, True),
    (13, 13, 128, 1, 0.1, 0.2, True),
    (36, 36, 32, 3, 0.1, 0.1, False),
    (12, 18, 100, 1, 0.3, 0.3, False),
    (9, 13, 70, 1, 0.1, 0.2, False),
    (17, 17, 128, 1, 0.1, 0.2, True),
    (16, 5, 100, 2, 0.3, 0.3, False),
    (84, 84, 64, 2, 0.1, 0.2, False),
    (6, 13, 128, 1, 1.0, 0.5, False),
]


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("A,B,T,d,h,scale,yx", SOAK_REGIMES)
def test_soak_regimes_default_dispatch(gpu, A, B, T, d, h, scale, yx, seed):
    """every launch form of the default dispatch (Gram + gradient, forward only, the sharded partial solve) per entry"""
    from sigsvgd_amd import ops

    X = walks(A, T, d, 100 * T + 10 * d + seed, scale)
    Y = X if yx else walks(B, T, d, 100 * T + 10 * d + seed + 5, scale)
    go = np.random.default_rng(seed).uniform(0.5, 1.5, (A, B)).astype(np.float32)
    Kref, gref = C.gram_fwd_bwd(X, Y, h, 0, grad_out=go.astype(np.float64))
    Xg, gog = torch.as_tensor(X, device=gpu), torch.as_tensor(go, device=gpu)
    Yg = Xg if yx else torch.as_tensor(Y, device=gpu)
    K, g = ops.gram_fwd_bwd(Xg, Yg, 1.0 / h, grad_out=gog, y_is_x=yx)
    Kf = ops.gram_fwd(Xg, Yg, 1.0 / h, y_is_x=yx)
    torch.cuda.synchronize()
    assert rel_entry(K.cpu().numpy(), Kref, 1e-6) < TOL
    assert rel_entry(Kf.cpu().numpy(), Kref, 1e-6) < TOL
    assert rel_max(g.cpu().numpy(), gref) < TOL
    if yx:
        Ks = torch.zeros(A, A, device=gpu)
        gs = torch.zeros(A, T, d, device=gpu, dtype=torch.float64)
        for r in range(2):
            Kp, gp = ops.gram_sym_partial(Xg, 1.0 / h, r, 2, grad_out=gog, fold=True)
            Ks += Kp
            gs += gp
        assert rel_entry(Ks.cpu().numpy(), Kref, 1e-6) < TOL
        assert rel_max(gs.cpu().numpy(), gref) < TOL


@pytest.mark.parametrize("h", [0.02, 0.1, 0.5, 1.0])
@pytest.mark.parametrize("scale", [0.1, 0.2, 0.5])
@pytest.mark.parametrize("N,T", [(12, 64), (10, 100), (12, 32)])
def test_one_channel_sweep_rows(gpu, N, T, scale, h):
    """the d = 1 rows of the roughness x bandwidth sweep where the discrete solution oscillates (round 3: up to 1.9e-5)"""
    from sigsvgd_amd import ops

    X = walks(N, T, 1, 0, scale)
    Kref, gref = C.gram_fwd_bwd(X, X, h, 0)
    if not np.isfinite(Kref).all() or np.abs(Kref).max() > 1e30:
        pytest.skip("K beyond the fp32 range: no fp32 answer exists")
    Xg = torch.as_tensor(X, device=gpu)
    for sym in (True, False):
        K, g = ops.gram_fwd_bwd(Xg, Xg if sym else Xg.clone(), 1.0 / h, y_is_x=sym)
        assert rel_entry(K.cpu().numpy(), Kref, 1e-6) < TOL
        assert rel_max(g.cpu().numpy(), gref) < TOL
        assert rel_entry(ops.gram_fwd(Xg, Xg if sym else Xg.clone(), 1.0 / h, y_is_x=sym).cpu().numpy(), Kref, 1e-6) < TOL


@pytest.mark.parametrize("N,T,d", [(64, 64, 3), (48, 64, 1), (40, 100, 3), (64, 32, 2)])
def test_smooth_few_channel_launches_flag_nothing(gpu, N, T, d):
    """the conditioning rule must not send well-conditioned pairs to the fp64 pass: on the bench inputs (step 0.05, h = 1) the
    default dispatch and the same launch with every pair forced through the coverage kernel agree to fp32 resolution, and the
    default result carries the fp32 route's own last bits (it differs from the fp64 pass's somewhere: nothing was replaced)"""
    from oracle import sigkernel_oracle as O
    from sigsvgd_amd import ops

    X, _ = O.synthetic_inputs(N, T, d)
    Xg = X.to(gpu)
    K = ops.gram_fwd(Xg, Xg, 1.0, y_is_x=True)
    Kx = ops.gram_fwd(Xg, Xg, 1.0, y_is_x=True, force_generic=True)
    torch.cuda.synchronize()
    assert rel_entry(K.cpu().numpy(), Kx.double().cpu().numpy(), 1e-6) < 3e-6
    same = (K == Kx).float().mean().item()
    assert same < 0.9, same  # (an exact pass over every pair would make the two identical)


@pytest.mark.parametrize("A,B,T,d,h,scale", [(16, 5, 100, 2, 0.3, 0.3), (6, 4, 128, 14, 1.0, 0.05), (5, 7, 128, 16, 1.0, 0.08),
                                             (7, 7, 120, 1, 0.1, 0.2), (4, 6, 150, 3, 1.0, 0.05)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_exact_pass_long_paths(gpu, A, B, T, d, h, scale, dtype):
    """force_generic with the gradient beyond T ~ 92: round 3's coverage kernel fell back to fp32 increments there (soak case
    3027: 2.9e-5).  The long-path layout now forms the increments per band in fp64: 1e-7 (fp32 I/O) / 1e-11 (fp64 I/O) with and
    without the gradient, symmetric and ordered."""
    from sigsvgd_amd import ops

    X, Y = walks(A, T, d, 3, scale), walks(B, T, d, 4, scale)
    go = np.random.default_rng(5).uniform(0.5, 1.5, (A, B))
    Kref, gref = C.gram_fwd_bwd(X, Y, h, 0, grad_out=go)
    Xg, Yg, gog = (torch.as_tensor(t, device=gpu).to(dtype) for t in (X, Y, go))
    tol = 2e-7 if dtype == torch.float32 else 1e-10
    K, g = ops.gram_fwd_bwd(Xg, Yg, 1.0 / h, grad_out=gog, force_generic=True)
    Kf = ops.gram_fwd(Xg, Yg, 1.0 / h, force_generic=True)
    torch.cuda.synchronize()
    assert rel_entry(K.cpu().numpy(), Kref, 1e-6) < tol
    assert rel_entry(Kf.cpu().numpy(), Kref, 1e-6) < tol
    assert rel_max(g.cpu().numpy(), gref) < 1e-6  # (the stored forward solution and S are fp32 whatever the I/O type)
    if A == B:
        Ks, gs = ops.gram_fwd_bwd(Xg, Xg, 1.0 / h, y_is_x=True, force_generic=True)
        Kr2, gr2 = C.gram_fwd_bwd(X, X, h, 0)
        assert rel_entry(Ks.cpu().numpy(), Kr2, 1e-6) < tol
        assert rel_max(gs.cpu().numpy(), gr2) < 1e-6


def test_linear_kernel_on_refined_shapes_fresh_workspace(gpu):
    """the workspace query sized refined shapes for the refined-grid / band kernels whatever the static
    kernel, while the linear kernel runs them on the coverage kernel (far more scratch).  The query takes the static kind
    since ABI 9; a launch on a workspace of exactly the queried size must pass -- here between the guards of
    tests/guarded_workspace.py, every byte 0xFF, at the worst alignment (tests/test_gpu_workspace.py does that for every
    launch form)."""
    import ctypes

    from guarded_workspace import GuardedWorkspace
    from oracle import sigkernel_oracle as O
    from sigsvgd_amd import _lib, ops

    L = _lib.load()
    for (A, B, T, d, n) in [(9, 7, 30, 3, 2), (9, 7, 30, 3, 3), (6, 6, 20, 2, 0), (5, 5, 100, 2, 0)]:
        X, Y = walks(A, T, d, 1, 0.05), walks(B, T, d, 2, 0.05)
        Kref, gref = O.gram_backward(X.astype(np.float64), Y.astype(np.float64), None, O.LINEAR, 1.0, n)
        Xg, Yg = torch.as_tensor(X, device=gpu), torch.as_tensor(Y, device=gpu)
        nb = ctypes.c_size_t(0)
        assert L.sigsvgd_gram_workspace_bytes(A, B, T, d, n, _lib.STATIC_LINEAR, 1, 0, ctypes.byref(nb)) == 0
        guarded = GuardedWorkspace("ones", 1)
        ws, nws = guarded(gpu, nb.value)
        assert nws == nb.value and ws.numel() == nb.value
        K = torch.empty(A, B, device=gpu)
        g = torch.empty(A, T, d, device=gpu)
        rc = L.sigsvgd_gram_fwd_bwd(Xg.data_ptr(), Yg.data_ptr(), A, B, T, d, _lib.F32, 1.0, n, _lib.STATIC_LINEAR, 0, None,
                                    K.data_ptr(), g.data_ptr(), ws.data_ptr(), nws, None)
        assert rc == 0, _lib.last_error()
        torch.cuda.synchronize()
        guarded.check()
        assert rel_entry(K.cpu().numpy(), Kref, 1e-6) < TOL and rel_max(g.cpu().numpy(), gref) < TOL
        K2, g2 = ops.gram_fwd_bwd(Xg, Yg, 1.0, n, static_kind=_lib.STATIC_LINEAR)
        assert torch.equal(K, K2) and torch.equal(g, g2)


def _probe_paths(A, T, d, scale, h):
    """the inputs of one row of profiles/r04_smooth_one_channel.txt: scripts/dev/smooth_one_channel.py drew every row from ONE
    generator (seed 3) in the order of its loops, so a row's paths are replayed by drawing (and dropping) the rows before it"""
    rng = np.random.default_rng(3)
    for (a, t, dd, _n) in [(20, 64, 1, 0), (20, 33, 1, 0), (12, 128, 1, 0), (12, 100, 2, 0), (20, 33, 1, 1), (20, 17, 1, 2),
                           (20, 64, 2, 0), (20, 5, 1, 4), (16, 9, 1, 3), (20, 20, 1, 0)]:
        for (s, hh) in [(0.02, 10.0), (0.01, 10.0), (0.02, 4.0)]:
            X = np.cumsum(s * rng.standard_normal((a, t, dd)), axis=1).astype(np.float32)
            if (a, t, dd, _n, s, hh) == (A, T, d, 0, scale, h):
                return X
    raise ValueError("not a row of the probe")


def _parity_all_forms(gpu, X, Y, h, seed, partial=False, ones=True):
    """the launch forms of test_soak_regimes_default_dispatch on one input: Gram + gradient with a random grad_out (symmetric
    on X, ordered on X against Y) and, with `ones`, with grad_out = None; forward only (both); with `partial` the sharded
    symmetric solve over 2 ranks, folded.
    Returns the errors by form; K per entry (_relK), the gradient over its largest entry (_rel)."""
    from sigsvgd_amd import ops

    A, B = X.shape[0], Y.shape[0]
    rng = np.random.default_rng(seed)
    go_s = rng.uniform(0.5, 1.5, (A, A)).astype(np.float32)
    go_o = rng.uniform(0.5, 1.5, (A, B)).astype(np.float32)
    Ks_ref, gs_ref = C.gram_fwd_bwd(X, X, h, 0, grad_out=go_s.astype(np.float64))
    Ko_ref, go_ref = C.gram_fwd_bwd(X, Y, h, 0, grad_out=go_o.astype(np.float64))
    Xg, Yg = torch.as_tensor(X, device=gpu), torch.as_tensor(Y, device=gpu)
    gsg, gog = torch.as_tensor(go_s, device=gpu), torch.as_tensor(go_o, device=gpu)
    K, g = ops.gram_fwd_bwd(Xg, Xg, 1.0 / h, grad_out=gsg, y_is_x=True)
    Ko, go = ops.gram_fwd_bwd(Xg, Yg, 1.0 / h, grad_out=gog)
    Kf = ops.gram_fwd(Xg, Xg, 1.0 / h, y_is_x=True)
    Kfo = ops.gram_fwd(Xg, Yg, 1.0 / h)
    torch.cuda.synchronize()
    err = {"sym K": rel_entry(K.cpu().numpy(), Ks_ref, 1e-6), "sym grad": rel_max(g.cpu().numpy(), gs_ref),
           "ordered K": rel_entry(Ko.cpu().numpy(), Ko_ref, 1e-6), "ordered grad": rel_max(go.cpu().numpy(), go_ref),
           "fwd sym K": rel_entry(Kf.cpu().numpy(), Ks_ref, 1e-6), "fwd ordered K": rel_entry(Kfo.cpu().numpy(), Ko_ref, 1e-6)}
    if ones:  # grad_out = None: the gradient sums the partners with equal weights and can cancel far below the weighted one's
        for name, Z, Zg, yx in (("ones sym", X, Xg, True), ("ones ordered", Y, Yg, False)):
            K1_ref, g1_ref = C.gram_fwd_bwd(X, Z, h, 0)
            K1, g1 = ops.gram_fwd_bwd(Xg, Zg, 1.0 / h, y_is_x=yx)
            torch.cuda.synchronize()
            err[name + " K"] = rel_entry(K1.cpu().numpy(), K1_ref, 1e-6)
            err[name + " grad"] = rel_max(g1.cpu().numpy(), g1_ref)
    if partial:
        Kp = torch.zeros(A, A, device=gpu)
        gp = torch.zeros(X.shape, device=gpu, dtype=torch.float64)
        for r in range(2):
            k_r, g_r = ops.gram_sym_partial(Xg, 1.0 / h, r, 2, grad_out=gsg, fold=True)
            Kp += k_r
            gp += g_r
        torch.cuda.synchronize()
        err["partial K"] = rel_entry(Kp.cpu().numpy(), Ks_ref, 1e-6)
        err["partial grad"] = rel_max(gp.cpu().numpy(), gs_ref)
    return err


# (A, T, d, step, h): very smooth paths in one channel at dyadic order 0 -- |step|^2 / h ~ 1e-5 .. 4e-5, K = 1 + O(1e-4), the
# gradient O(1e-4) of K.  The first three are the rows of profiles/r04_smooth_one_channel.txt beyond 1e-5 (33 and 20 points:
# two pairs per wavefront on the register-resident kernel; 128 points: quadrant kernel), the others their neighbours that
# were inside it (64 and 100 points in one channel, 33 points in two).
SMOOTH_ONE_CHANNEL = [
    (20, 33, 1, 0.01, 10.0),
    (20, 20, 1, 0.02, 10.0),
    (12, 128, 1, 0.01, 10.0),
    (20, 64, 1, 0.01, 10.0),
    (12, 100, 1, 0.01, 10.0),
    (20, 33, 2, 0.01, 10.0),
]


@pytest.mark.parametrize("A,T,d,step,h,src", [c + ("probe",) for c in SMOOTH_ONE_CHANNEL[:4]]
                         + [c + (seed,) for c in SMOOTH_ONE_CHANNEL for seed in (0, 1)])
def test_smooth_one_channel_order0(gpu, A, T, d, step, h, src):
    """K and the gradient of very smooth few-channel paths, every launch form, within 1e-5 ("very smooth
    paths in one channel").  src "probe": the exact inputs of the r04 probe row (before the one-channel gradient launches went
    to the coverage kernel: 1.97e-5, 1.20e-5, 1.24e-5 for the first three, all with grad_out = None); an int: a fixed seed."""
    if src == "probe":
        X = _probe_paths(A, T, d, step, h)
    else:
        X = walks(A, T, d, 1000 * T + 10 * d + src, step)
    Y = X.copy()  # the ordered launch: Y a separate tensor with X's values (the probe's form)
    err = _parity_all_forms(gpu, X, Y, h, 7 + (0 if src == "probe" else src))
    assert max(err.values()) < TOL, err


@pytest.mark.parametrize("h", [0.1, 0.3, 1.0])
@pytest.mark.parametrize("step", [0.2, 0.5])
@pytest.mark.parametrize("T", [32, 64, 100, 128])
@pytest.mark.parametrize("d", [5, 8, 9, 14, 16])
def test_rough_wide_paths_default_dispatch(gpu, d, T, step, h):
    """rough paths in 5 .. 16 channels on the default dispatch, every launch form: the ends of the 8-channel instantiations
    (5, 8), the first 16-channel one (9), both sides of the quadrant kernel's ROWG split (14, 16); T = 32 / 64 on the
    register-resident kernel (two pairs per wavefront at 32), T = 100 / 128 on the quadrant kernel.  These kernels flag no pair
    for conditioning (the 8- and 16-channel register-resident instantiations have no exact pass at all, only the fp64 re-sweep
    of a cancelled pair), so this is what holds them to 1e-5 where the discrete solution oscillates and K is large."""
    A, B = 12, 9
    X = walks(A, T, d, 10000 + 100 * d + T, step)
    Y = walks(B, T, d, 20000 + 100 * d + T, step)
    Kref = np.concatenate([C.gram_fwd_bwd(X, X, h, 0, want_grad=False)[0], C.gram_fwd_bwd(X, Y, h, 0, want_grad=False)[0]], 1)
    if not np.isfinite(Kref).all() or np.abs(Kref).max() > 1e30:
        pytest.skip("K beyond the fp32 range: no fp32 answer exists")
    err = _parity_all_forms(gpu, X, Y, h, 11, partial=True, ones=False)
    assert max(err.values()) < TOL, err


@pytest.mark.parametrize("yx", [True, False])
def test_third_caller_order3_coverage(gpu, yx):
    """the reference's third caller (examples/test_optimise_arm_spline-with-path-signature.py upstream): [6, 100, 3] paths at
    dyadic order 3, Gram + gradient -- a refined grid of 792 cells per side, beyond the band kernel: the coverage kernel"""
    from sigsvgd_amd import ops

    h = 1.0
    X = walks(6, 100, 3, 31, 0.05)
    Y = X if yx else walks(6, 100, 3, 32, 0.05)
    go = np.random.default_rng(33).uniform(0.5, 1.5, (6, 6)).astype(np.float32)
    Kref, gref = C.gram_fwd_bwd(X, Y, h, 3, grad_out=go.astype(np.float64))
    Xg, gog = torch.as_tensor(X, device=gpu), torch.as_tensor(go, device=gpu)
    Yg = Xg if yx else torch.as_tensor(Y, device=gpu)
    K, g = ops.gram_fwd_bwd(Xg, Yg, 1.0 / h, 3, grad_out=gog, y_is_x=yx)
    Kf = ops.gram_fwd(Xg, Yg, 1.0 / h, 3, y_is_x=yx)
    torch.cuda.synchronize()
    assert rel_entry(K.cpu().numpy(), Kref, 1e-6) < TOL
    assert rel_entry(Kf.cpu().numpy(), Kref, 1e-6) < TOL
    assert rel_max(g.cpu().numpy(), gref) < TOL
