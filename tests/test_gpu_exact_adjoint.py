"""SIGSVGD_FLAG_EXACT_ADJOINT on the device: every gradient launch of the long route against the fp64
helper of tests/exact_adjoint_reference.py (which tests/test_exact_adjoint_cpu.py holds to central differences of its own K),
at the edges of the ring sweep:

    P = 63 / 64 / 65 and 128 / 129   the band hand-over of h through rowbuf, the last band shorter than 64 rows (down to 1)
    Q = 1, 7, 8, 9                   the 8-deep ring of the stored forward values in the reverse sweep
    TX != TY, orders 1 and 2         block sums over r columns (in the lane) and r rows (ring_S)
    order 7 with T = 3               nrow = 1: a band inside one coarse row
    T = 131 at order 0               the increment ring refilled inside a band, W capped at 128 columns

Each case asserts, in this order: the library takes the flag (a library without the feature answers SIGSVGD_E_BADARG, which
`ops` raises); K has the bits of the unflagged launch; the gradients and dK_dinvh are within BOUND of the helper; a second call
returns the same bits; and NAIVE | EXACT returns the bits of NAIVE in every output.

BOUND = 1e-5 of the largest entry is what tests/test_gpu_long.py, test_gpu_long2.py, test_gpu_pair.py and test_gpu_matern.py
hold the GG gradients of the same kernels to against the oracle: the stored c and S are fp32 here as K00 and S are there.
Measured on the MI355X (profiles/exact_adjoint.txt): worst ratio 2.8e-6 over every case of this file (dK_dinvh of the paired
bandwidth launch at T = 131 with fp32 I/O), 1.3e-6 for a coordinate gradient, most figures between 4e-8 and 4e-7.

The paths hold fp32 values, so fp32 and fp64 I/O see the same inputs; they are rough (steps of 0.5 per channel at bandwidth 1)
so that GG is per cents away from the exact gradient (test_flag_changes_the_gradient; tests/test_exact_adjoint_cpu.py)."""
import numpy as np
import pytest
import torch

import exact_adjoint_reference as E
from parity import np64, rel_max, signed_weights

pytestmark = pytest.mark.gpu

BOUND = 1e-5
F64, F32 = torch.float64, torch.float32

# name -> (A, B, TX, TY, d, n)
SHAPES = {
    "P63_Q1": (2, 3, 64, 2, 1, 0),
    "P64_Q7": (3, 2, 65, 8, 3, 0),
    "P65_Q8": (2, 2, 66, 9, 7, 0),
    "P128_Q9": (2, 3, 129, 10, 3, 0),
    "P129_Q8": (2, 2, 130, 9, 3, 0),
    "order1_P64_Q10": (3, 2, 33, 6, 3, 1),
    "order2_P68_Q16": (2, 2, 18, 5, 3, 2),
    "order7_T3": (2, 2, 3, 3, 2, 7),
    "T131": (2, 2, 131, 131, 2, 0),
    "Q130_A5": (5, 2, 4, 131, 3, 0),
}
CASES = [(name, F64) for name in SHAPES] + [("P65_Q8", F32), ("T131", F32)]
SQUARE = {"T131": (2, 2, 131, 131, 2, 0), "order2_T18": (3, 3, 18, 18, 3, 2), "P65_A4": (4, 4, 66, 66, 1, 0)}
NAIVE_KINDS = (E.RBF, E.LINEAR)  # (the other kinds have the default stencil only on the long route)


def rough(seed, B, T, d, kind=E.RBF):
    """[B, T, d] fp32-valued walks with steps of 0.5 per channel (0.12 for the linear kernel, whose increments are not bounded
    by 1: K stays of order 1 to 1e3)"""
    rng = np.random.default_rng(seed)
    step = 0.12 if kind == E.LINEAR else 0.5
    return np.cumsum(step * rng.standard_normal((B, T, d)), axis=1).astype(np.float32).astype(np.float64)


def inputs(name, kind=E.RBF, shapes=SHAPES):
    A, B, TX, TY, d, n = shapes[name]
    seed = sum(map(ord, name)) + 17 * kind
    return rough(seed, A, TX, d, kind), rough(seed + 1, B, TY, d, kind), n


def dev(a, io, gpu):
    return None if a is None else torch.as_tensor(a, dtype=io, device=gpu)


def same_bits(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


WORST = {}


def check(what, got, ref):
    """got within BOUND of ref (of its largest entry); the figure is printed and kept for the summary line"""
    err = rel_max(np64(got), ref)
    WORST[what] = max(WORST.get(what, 0.0), err)
    print(f"    {what}: {err:.2e} of the largest entry")
    assert err < BOUND, (what, err)


def run_protocol(launch, refs, naive_ok):
    """the five assertions of the module docstring on launch(exact_adjoint=..., naive=...) -> tuple of tensors (K first)"""
    out = launch(exact_adjoint=True, naive=False)  # 1: a library without the flag raises here (rc = SIGSVGD_E_BADARG)
    plain = launch(exact_adjoint=False, naive=False)
    assert torch.equal(out[0], plain[0])  # 2: K bit for bit
    for (what, ref), got in zip(refs, out[1:]):  # 3
        if ref is not None:
            check(what, got, ref)
    assert same_bits(out, launch(exact_adjoint=True, naive=False))  # 4
    if naive_ok:  # 5
        assert same_bits(launch(exact_adjoint=True, naive=True), launch(exact_adjoint=False, naive=True))
    return out, plain


# ---- sigsvgd_pde_fwd_bwd ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,io", CASES, ids=[f"{n}-{'f64' if io == F64 else 'f32'}" for n, io in CASES])
def test_pde_fwd_bwd(gpu, name, io):
    from sigsvgd_amd import ops

    A, B, M, N, _, n = SHAPES[name]
    rng = np.random.default_rng(M * 1000 + N)
    npairs = A + B
    G = (0.9 / np.sqrt(max(M, N)) * rng.standard_normal((npairs, M, N))).astype(np.float32).astype(np.float64)
    w = signed_weights(1, npairs, M + N)[0]
    _, _, R = E.pde(G, n)
    Gt, wt = dev(G, io, gpu), dev(w, io, gpu)
    launch = lambda exact_adjoint, naive: ops.pde_fwd_bwd(Gt, n, wt, naive, exact_adjoint=exact_adjoint)
    out, _ = run_protocol(launch, [("pde dG", w[:, None, None] * R)], True)
    assert torch.equal(out[0], ops.pde_fwd(Gt, n))


# ---- sigsvgd_gram_long_fwd_bwd ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,io", CASES, ids=[f"{n}-{'f64' if io == F64 else 'f32'}" for n, io in CASES])
def test_gram_long_fwd_bwd(gpu, name, io):
    from sigsvgd_amd import ops

    X, Y, n = inputs(name)
    w = signed_weights(len(X), len(Y), n + len(X))
    _, gX, _ = E.gram_backward(X, Y, w, E.RBF, 1.0, n)
    Xt, Yt, wt = dev(X, io, gpu), dev(Y, io, gpu), dev(w, io, gpu)
    launch = lambda exact_adjoint, naive: ops.gram_long_fwd_bwd(Xt, Yt, 1.0, n, E.RBF, wt, naive, exact_adjoint=exact_adjoint)
    run_protocol(launch, [("long gX", gX)], True)


def test_gram_long_fwd_bwd_sym(gpu):
    from sigsvgd_amd import ops

    X, _, n = inputs("order2_T18", shapes=SQUARE)
    w = signed_weights(len(X), len(X), 5)
    _, gX, _ = E.gram_backward(X, X, w, E.RBF, 1.0, n, sym=True)
    Xt, wt = dev(X, F64, gpu), dev(w, F64, gpu)
    launch = lambda exact_adjoint, naive: ops.gram_long_fwd_bwd(Xt, Xt, 1.0, n, E.RBF, wt, naive, True,
                                                                exact_adjoint=exact_adjoint)
    run_protocol(launch, [("long gX sym", gX)], True)


def test_flag_changes_the_gradient(gpu):
    """the unflagged launch is GG: per cents away from the exact gradient on these paths (so the cases here cannot pass on it)"""
    from sigsvgd_amd import ops

    X, Y, n = inputs("P128_Q9")
    Xt, Yt = dev(X, F64, gpu), dev(Y, F64, gpu)
    _, g_gg = ops.gram_long_fwd_bwd(Xt, Yt, 1.0, n)
    _, g_ex = ops.gram_long_fwd_bwd(Xt, Yt, 1.0, n, exact_adjoint=True)
    assert rel_max(np64(g_gg), np64(g_ex)) > 1e-2


# ---- sigsvgd_gram_long_fwd_bwd2 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,io", CASES, ids=[f"{n}-{'f64' if io == F64 else 'f32'}" for n, io in CASES])
def test_gram_long_fwd_bwd2_both_gradients(gpu, name, io):
    from sigsvgd_amd import ops

    X, Y, n = inputs(name)
    w = signed_weights(len(X), len(Y), n + 3)
    _, gX, gY = E.gram_backward(X, Y, w, E.RBF, 1.0, n)
    Xt, Yt, wt = dev(X, io, gpu), dev(Y, io, gpu), dev(w, io, gpu)
    launch = lambda exact_adjoint, naive: ops.gram_long_fwd_bwd2(Xt, Yt, 1.0, n, E.RBF, wt, naive,
                                                                 exact_adjoint=exact_adjoint)
    run_protocol(launch, [("long2 gX", gX), ("long2 gY", gY)], True)


@pytest.mark.parametrize("mode", ["y_is_x", "sym", "y_is_x+sym", "gY_only"])
@pytest.mark.parametrize("name", list(SQUARE))
def test_gram_long_fwd_bwd2_modes(gpu, name, mode):
    from sigsvgd_amd import ops

    X, Y, n = inputs(name, shapes=SQUARE)
    yx, sym = "y_is_x" in mode, "sym" in mode
    if yx:
        Y = X
    w = signed_weights(len(X), len(Y), 11)
    _, gX, gY = E.gram_backward(X, Y, w, E.RBF, 1.0, n, sym=sym)
    Xt, Yt, wt = dev(X, F64, gpu), dev(Y, F64, gpu), dev(w, F64, gpu)
    want_x = mode != "gY_only"
    launch = lambda exact_adjoint, naive: ops.gram_long_fwd_bwd2(Xt, Xt if yx else Yt, 1.0, n, E.RBF, wt, naive, sym, yx, want_x,
                                                                 True, exact_adjoint=exact_adjoint)
    refs = [("long2 gX " + mode, gX if want_x else None), ("long2 gY " + mode, None if (yx or sym) else gY)]
    out, _ = run_protocol(launch, refs, True)
    assert (out[1] is None) == (not want_x) and (out[2] is None) == (yx or sym)


@pytest.mark.parametrize("kind", E.KINDS)
@pytest.mark.parametrize("name", ["P65_Q8", "order1_P64_Q10"])
def test_gram_long_fwd_bwd2_kinds(gpu, name, kind):
    from sigsvgd_amd import ops

    X, Y, n = inputs(name, kind)
    w = signed_weights(len(X), len(Y), kind)
    _, gX, gY = E.gram_backward(X, Y, w, kind, 1.0, n)
    Xt, Yt, wt = dev(X, F64, gpu), dev(Y, F64, gpu), dev(w, F64, gpu)
    launch = lambda exact_adjoint, naive: ops.gram_long_fwd_bwd2(Xt, Yt, 1.0, n, kind, wt, naive, exact_adjoint=exact_adjoint)
    run_protocol(launch, [(f"long2 gX kind {kind}", gX), (f"long2 gY kind {kind}", gY)], kind in NAIVE_KINDS)


# ---- sigsvgd_pair_fwd_bwd --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,io", CASES, ids=[f"{n}-{'f64' if io == F64 else 'f32'}" for n, io in CASES])
def test_pair_fwd_bwd(gpu, name, io):
    from sigsvgd_amd import ops

    X, Y, n = inputs(name)
    A = min(len(X), len(Y))
    X, Y = X[:A], Y[:A]
    w = signed_weights(1, A, n + 7)[0]
    _, gX, gY = E.pair_backward(X, Y, w, E.RBF, 1.0, n)
    Xt, Yt, wt = dev(X, io, gpu), dev(Y, io, gpu), dev(w, io, gpu)
    launch = lambda exact_adjoint, naive: ops.pair_fwd_bwd(Xt, Yt, 1.0, n, E.RBF, wt, naive, exact_adjoint=exact_adjoint)
    out, _ = run_protocol(launch, [("pair gX", gX), ("pair gY", gY)], True)
    assert torch.equal(out[0], ops.pair_fwd(Xt, Yt, 1.0, n))


@pytest.mark.parametrize("kind", E.KINDS)
@pytest.mark.parametrize("name", ["P129_Q8", "order2_P68_Q16"])
def test_pair_fwd_bwd_kinds(gpu, name, kind):
    from sigsvgd_amd import ops

    X, Y, n = inputs(name, kind)
    _, gX, gY = E.pair_backward(X, Y, None, kind, 1.0, n)
    Xt, Yt = dev(X, F64, gpu), dev(Y, F64, gpu)
    launch = lambda exact_adjoint, naive: ops.pair_fwd_bwd(Xt, Yt, 1.0, n, kind, None, naive, exact_adjoint=exact_adjoint)
    run_protocol(launch, [(f"pair gX kind {kind}", gX), (f"pair gY kind {kind}", gY)], kind in NAIVE_KINDS)


def test_pair_runs_one_wave_per_pair_with_the_flag(gpu, monkeypatch):
    """a launch pinned to the band-parallel schedule runs the one-wavefront kernel with the flag: same K, the exact gradient"""
    from sigsvgd_amd import ops

    monkeypatch.setenv("SIGSVGD_PAIR_MODE", "bands")
    X, Y, n = inputs("P129_Q8")
    assert ops.pair_schedule(len(X), X.shape[1], Y.shape[1], X.shape[2], n)[0] > 1
    assert ops.pair_schedule(len(X), X.shape[1], Y.shape[1], X.shape[2], n, exact_adjoint=True)[0] == 1
    _, gX, gY = E.pair_backward(X, Y, None, E.RBF, 1.0, n)
    Xt, Yt = dev(X, F64, gpu), dev(Y, F64, gpu)
    launch = lambda exact_adjoint, naive: ops.pair_fwd_bwd(Xt, Yt, 1.0, n, E.RBF, None, naive, exact_adjoint=exact_adjoint)
    run_protocol(launch, [("pair gX (bands pinned)", gX), ("pair gY (bands pinned)", gY)], True)


# ---- the bandwidth launches ------------------------------------------------------------------------------------------------------
H_CASES = [("P64_Q7", E.RBF, F64), ("P129_Q8", E.RBF, F64), ("order2_P68_Q16", E.RBF, F64), ("T131", E.RBF, F32),
           ("P65_Q8", E.IMQ, F64), ("P65_Q8", E.RQ, F64), ("order1_P64_Q10", E.MATERN32, F64), ("P128_Q9", E.MATERN52, F64)]


@pytest.mark.parametrize("name,kind,io", H_CASES, ids=[f"{n}-kind{k}-{'f64' if io == F64 else 'f32'}" for n, k, io in H_CASES])
def test_gram_long_fwd_bwd_h(gpu, name, kind, io):
    from sigsvgd_amd import ops

    X, Y, n = inputs(name, kind)
    w = signed_weights(len(X), len(Y), 3)
    _, gX, gY = E.gram_backward(X, Y, w, kind, 1.0, n)
    dK = E.dK_dinvh(X, Y, kind, 1.0, n)
    Xt, Yt, wt = dev(X, io, gpu), dev(Y, io, gpu), dev(w, io, gpu)
    launch = lambda exact_adjoint, naive: ops.gram_long_fwd_bwd_h(Xt, Yt, 1.0, n, kind, wt, naive,
                                                                  exact_adjoint=exact_adjoint)
    out, _ = run_protocol(launch, [("long_h gX", gX), ("long_h gY", gY), ("long_h dK_dinvh", dK)], kind in NAIVE_KINDS)
    # the coordinate gradients have the bits of the launch without the bandwidth pass
    assert same_bits(out[:3], ops.gram_long_fwd_bwd2(Xt, Yt, 1.0, n, kind, wt, exact_adjoint=True))


@pytest.mark.parametrize("name,kind,io", H_CASES, ids=[f"{n}-kind{k}-{'f64' if io == F64 else 'f32'}" for n, k, io in H_CASES])
def test_pair_fwd_bwd_h(gpu, name, kind, io):
    from sigsvgd_amd import ops

    X, Y, n = inputs(name, kind)
    A = min(len(X), len(Y))
    X, Y = X[:A], Y[:A]
    _, gX, gY = E.pair_backward(X, Y, None, kind, 1.0, n)
    dK = E.pair_dK_dinvh(X, Y, kind, 1.0, n)
    Xt, Yt = dev(X, io, gpu), dev(Y, io, gpu)
    launch = lambda exact_adjoint, naive: ops.pair_fwd_bwd_h(Xt, Yt, 1.0, n, kind, None, naive, exact_adjoint=exact_adjoint)
    run_protocol(launch, [("pair_h gX", gX), ("pair_h gY", gY), ("pair_h dK_dinvh", dK)], kind in NAIVE_KINDS)


def test_gram_long_fwd_bwd_h_y_is_x(gpu):
    from sigsvgd_amd import ops

    X, _, n = inputs("order2_T18", shapes=SQUARE)
    _, gX, _ = E.gram_backward(X, X, None, E.RBF, 1.0, n)
    dK = E.dK_dinvh(X, X, E.RBF, 1.0, n)
    Xt = dev(X, F64, gpu)
    launch = lambda exact_adjoint, naive: ops.gram_long_fwd_bwd_h(Xt, Xt, 1.0, n, E.RBF, None, naive, False, True,
                                                                  exact_adjoint=exact_adjoint)
    out, _ = run_protocol(launch, [("long_h gX y_is_x", gX), ("long_h gY", None), ("long_h dK_dinvh y_is_x", dK)], True)
    assert torch.equal(out[3], out[3].T)


# ---- the public surface, fp64 ----------------------------------------------------------------------------------------------------
SIGMA = 0.8


def surface_inputs(gpu, grad=True):
    X = torch.as_tensor(rough(91, 3, 20, 2), dtype=F64, device=gpu).requires_grad_(grad)
    Y = torch.as_tensor(rough(92, 3, 17, 2), dtype=F64, device=gpu).requires_grad_(grad)
    return X, Y


def test_sigkernel_compute_kernel(gpu):
    import sigsvgd_amd.sigkernel as sk

    X, Y = surface_inputs(gpu)
    w = torch.as_tensor(signed_weights(1, 3, 4)[0], device=gpu)
    (sk.SigKernel(sk.RBFKernel(SIGMA), 1, exact_grad=True).compute_kernel(X, Y) * w).sum().backward()
    _, gX, gY = E.pair_backward(np64(X), np64(Y), np64(w), E.RBF, SIGMA, 1)
    check("compute_kernel gX", X.grad, gX)
    check("compute_kernel gY", Y.grad, gY)


def test_sigkernel_compute_mmd_grad_y(gpu):
    import sigsvgd_amd.sigkernel as sk

    X, Y = surface_inputs(gpu)
    sk.SigKernel(sk.RBFKernel(SIGMA), 1, exact_grad=True).compute_mmd(X, Y, grad_Y=True).backward()
    Xn, Yn = np64(X), np64(Y)
    a, b = len(Xn), len(Yn)
    _, gxx, _ = E.gram_backward(Xn, Xn, np.full((a, a), 1.0 / (a * a)), E.RBF, SIGMA, 1, sym=True)
    _, gyy, _ = E.gram_backward(Yn, Yn, np.full((b, b), 1.0 / (b * b)), E.RBF, SIGMA, 1, sym=True)
    _, gx, gy = E.gram_backward(Xn, Yn, np.full((a, b), -2.0 / (a * b)), E.RBF, SIGMA, 1)
    check("compute_mmd gX", X.grad, gxx + gx)
    check("compute_mmd gY", Y.grad, gyy + gy)


def test_sigkernel_learned_sigma(gpu):
    """grad_sigma against the central difference in sigma of the helper's K (the weights make it a sum of signed terms)"""
    import sigsvgd_amd.sigkernel as sk

    X, Y = surface_inputs(gpu, grad=False)
    sigma = torch.tensor(SIGMA, dtype=F64, requires_grad=True)
    w = signed_weights(3, 3, 8)
    kernel = sk.SigKernel(sk.RBFKernel(sigma), 1, exact_grad=True)
    (kernel.compute_Gram(X, Y) * torch.as_tensor(w, device=gpu)).sum().backward()
    eps = 1e-6
    loss = lambda s: (w * E.gram(np64(X), np64(Y), E.RBF, s, 1)).sum()
    fd = (loss(SIGMA + eps) - loss(SIGMA - eps)) / (2 * eps)
    err = abs(float(sigma.grad) - fd) / abs(fd)
    print(f"    grad_sigma {float(sigma.grad):.9e} against {fd:.9e}: {err:.2e}")
    # the weighted terms dK_ij/dsigma have mixed signs; BOUND is of their largest, as for every other gradient here
    top = np.abs(w * E.dK_dinvh(np64(X), np64(Y), E.RBF, SIGMA, 1)).max() / SIGMA**2
    assert abs(float(sigma.grad) - fd) < BOUND * top + 1e-7 * abs(fd)  # (+ the truncation of the central difference)
    sigma.grad = None
    (kernel.compute_kernel(X, Y) * torch.as_tensor(w[0], device=gpu)).sum().backward()
    ref = -(w[0] * E.pair_dK_dinvh(np64(X), np64(Y), E.RBF, SIGMA, 1)).sum() / SIGMA**2
    assert abs(float(sigma.grad) - ref) < BOUND * np.abs(w[0] * E.pair_dK_dinvh(np64(X), np64(Y), E.RBF, SIGMA, 1)).max() / SIGMA**2


class UserRBF:
    """upstream's interface and nothing the package recognises: the grid is torch's, the PDE and its adjoint the device's"""

    def Gram_matrix(self, X, Y):
        d = X[:, None, :, None, :] - Y[None, :, None, :, :]
        return torch.exp(-(d * d).sum(-1) / SIGMA)


def test_sigkernel_user_static_kernel(gpu):
    import sigsvgd_amd.sigkernel as sk

    X, Y = surface_inputs(gpu)
    w = signed_weights(3, 3, 2)
    (sk.SigKernel(UserRBF(), 1, exact_grad=True).compute_Gram(X, Y) * torch.as_tensor(w, device=gpu)).sum().backward()
    _, gX, _ = E.gram_backward(np64(X), np64(Y), w, E.RBF, SIGMA, 1)
    check("user static kernel gX", X.grad, gX)
    assert Y.grad is None


def test_default_sigkernel_keeps_its_bits(gpu):
    """the default SigKernel runs the launches it ran (here the fused Gram kernel's, Y = X told): K and the GG gradient bit for
    bit `ops.gram_fwd_bwd`'s; exact_grad leaves the forward-only call alone and changes the gradient"""
    import sigsvgd_amd.sigkernel as sk
    from sigsvgd_amd import ops

    X, _ = surface_inputs(gpu)
    default, exact = sk.SigKernel(sk.RBFKernel(SIGMA), 1), sk.SigKernel(sk.RBFKernel(SIGMA), 1, exact_grad=True)
    K = default.compute_Gram(X, X)
    K.sum().backward()
    Kf, gf = ops.gram_fwd_bwd(X.detach(), X.detach(), 1.0 / SIGMA, 1, y_is_x=True)
    assert torch.equal(K.detach(), Kf) and torch.equal(X.grad, gf)
    Kd, gd = default.gram_and_grad(X.detach())
    assert torch.equal(Kd, Kf) and torch.equal(gd, gf)
    Xd = X.detach()  # (nothing requires grad: forward only)
    assert torch.equal(exact.compute_Gram(Xd, Xd), default.compute_Gram(Xd, Xd))
    _, ge = exact.gram_and_grad(X.detach())
    _, gx, _ = E.gram_backward(np64(X), np64(X), None, E.RBF, SIGMA, 1)
    check("gram_and_grad gX", ge, gx)
    assert rel_max(np64(gd), gx) > 1e-3


def test_worst_ratio_summary():
    """(runs last in the file: the largest ratio of every figure above, for profiles/exact_adjoint.txt)"""
    for what, err in sorted(WORST.items()):
        print(f"    worst {what}: {err:.2e}")
    if WORST:
        print(f"    worst of all: {max(WORST.values()):.2e} (bound {BOUND:.0e})")
