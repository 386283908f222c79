"""SIGSVGD_FLAG_NORMALIZED_FUSED on the device: the normalised kernel K^ and the first-slot gradient of
sum(w K^) from the fused Gram entry points, `ops.gram_fwd(..., normalized=True)` and `ops.gram_fwd_bwd(..., normalized=True)`,
against the fp64 restatement `log_k_reference.normalized_gram_and_grads`, and the surface built on it:
`SigKernel(normalize=True, normalize_route="fused")`, `kernels.SignatureKernel`, an `SVGD` step and `GraphedSigSVGD(normalize=True)`.

Inputs are fp32-valued walks (`log_k_reference.walks`), so both I/O types see the same numbers.  Every case first asserts on the
reference that every pair's and every diagonal's K is > 0 and that K(x, x) fits fp32; the seeds were chosen on the CPU for that
(SEED_BUMP) and no case is skipped.  Under Y_IS_X the reference's diagonal weights are set to zero, as
tests/test_gpu_normalized.py does.  The bounds:

    K^        per entry, relative: 1e-5, the fused route's own contract (tests/test_gpu_fast.py holds K to it), plus 3 * 2^-24
              with fp32 I/O for the two roundings (K_ij, then K_ij s_ij).  With Y_IS_X the diagonal is exactly 1 and K^ is
              bit-symmetric.
    gradient  1e-5 (max|t1| + max|t2|), t1 = sum_j w_ij s_ij d1 K_ij and t2 = 1/2 (sum_j U_ij) grad a_i, both on the reference
              (normalized_fused_reference.terms): the fused kernels hold a gradient to 1e-5 of its largest entry, and t2
              carries K's 1e-5 relative bound through U.  Not "1e-5 of the largest entry of the result": the result is a
              difference.  Each case asserts max(|t1|, |t2|) <= 2 max|result| on the reference, so the bound cannot hide a
              wrong result behind a large denominator.

Every launch runs a second time on a `GuardedWorkspace` of exactly the queried bytes, one byte off alignment, every byte 0xFF:
same bits, guards intact.  Each case prints the worst fraction of each bound (pytest -s).

On a library without the feature `ops.gram_fwd_bwd(normalized=True)` is a TypeError, and at the C level bit 4096 is ignored
and the unnormalised K comes back: every parity case fails."""
import functools

import numpy as np
import pytest
import torch

import log_k_reference as R
import normalized_fused_reference as NF
from guarded_workspace import GuardedWorkspace
from parity import np64, signed_weights
from sigsvgd_amd import _lib, ops

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
RBF, LINEAR, IMQ, M32 = _lib.STATIC_RBF, _lib.STATIC_LINEAR, _lib.STATIC_IMQ, _lib.STATIC_MATERN32
K_BOUND, G_BOUND = 1e-5, 1e-5

# name -> (A, B, T, d, n, kind, launch keywords, step): the smallest shapes that reach each route of the fused entry points and
# each edge of the two kernels around the pair solve (256 weights per block, 64 columns per pass of a row's wavefront)
SHAPES = {
    "fast_T9": (5, 4, 9, 3, 0, RBF, {}, 0.3),              # register-resident kernel, two rows per wavefront
    "fast_T40_d7": (3, 3, 40, 7, 0, RBF, {}, 0.3),
    "fast_T64_d2": (2, 3, 64, 2, 0, RBF, {}, 0.3),         # its last length
    "quad_T65": (2, 2, 65, 3, 0, RBF, {}, 0.3),            # quadrant kernel, first and last length
    "quad_T128": (2, 2, 128, 4, 0, RBF, {}, 0.2),
    "dyad_T17_n2": (3, 3, 17, 2, 2, RBF, {}, 0.3),         # refined grid, 64 cells
    "band_T10_n4": (3, 3, 10, 2, 4, RBF, {}, 0.3),         # bands: 144 cells
    "linear": (3, 2, 12, 3, 0, LINEAR, {}, 0.12),          # coverage kernel
    "imq": (3, 2, 12, 3, 0, IMQ, {}, 0.3),
    "imq_fp32": (3, 2, 12, 3, 0, IMQ, {"fp32_sweeps": True}, 0.3),
    "matern32": (3, 2, 12, 3, 0, M32, {}, 0.3),
    "forced": (3, 2, 12, 3, 0, RBF, {"force_generic": True}, 0.3),
    "one_channel": (3, 3, 20, 1, 0, RBF, {}, 0.3),
    "d17": (2, 2, 12, 17, 0, RBF, {}, 0.3),
    "B130": (3, 130, 5, 2, 0, RBF, {}, 0.3),               # three passes of the lane-stride loop, two weight blocks
    "A130": (130, 3, 5, 2, 0, RBF, {}, 0.3),
    "B63": (2, 63, 5, 2, 0, RBF, {}, 0.3),
    "B64": (2, 64, 5, 2, 0, RBF, {}, 0.3),
    "B65": (2, 65, 5, 2, 0, RBF, {}, 0.3),
    "N70": (70, 70, 5, 2, 0, RBF, {}, 0.3),                # Y_IS_X past one pass and 19 weight blocks
}
ALL_MODES = ("ordered", "sym", "yx", "yx_sym", "fwd", "yx_fwd")
SAME = ("yx", "yx_sym", "yx_fwd")
# name -> added to the seed, found on the CPU: the first choice has a pair with K <= 0 (quad_T128, N70) or a gradient whose two
# terms cancel past the ratio of 2 the reference is held to (band_T10_n4, one_channel)
SEED_BUMP = {"quad_T128": 1, "band_T10_n4": 1, "one_channel": 1, "N70": 1}


def modes_of(name):
    A, B = SHAPES[name][:2]
    if name == "N70":
        return ("yx", "yx_sym", "yx_fwd")
    return ALL_MODES if A == B else ("ordered", "fwd")


def inputs(name):
    A, B, T, d, n, kind, _, step = SHAPES[name]
    seed = sum(map(ord, name)) + SEED_BUMP.get(name, 0)
    X = R.walks(seed, A, T, d, step, np.float32).astype(np.float64)
    Y = R.walks(seed + 1000, B, T, d, step, np.float32).astype(np.float64)
    return X, Y


def weights(A, B, seed):
    """signed weights of order 1 with exact zeros (one at 2 x 2, so that both off-diagonal pairs are not without weight)"""
    w = signed_weights(A, B, seed).astype(np.float32).astype(np.float64)
    w[0, B - 1] = 0.0
    if A * B > 4:
        w[A - 1, 0] = 0.0
    return w


def reference(name, mode, unit=False):
    """-> (X, Y, w or None, K^, gradX or None, bound of the gradient) of a case in a mode; unit: grad_out = NULL.  Computed once
    and shared by the tests that need it."""
    return _reference(name, mode, bool(unit))


@functools.lru_cache(maxsize=None)
def _reference(name, mode, unit):
    A, B, T, d, n, kind, _, _ = SHAPES[name]
    X, Y = inputs(name)
    same, sym, fwd = mode in SAME, mode.endswith("sym"), mode.endswith("fwd")
    Y = X.copy() if same else Y
    a = R.log_pair_backward(X, X, None, kind, 1.0, n)[0]
    b = a if same else R.log_pair_backward(Y, Y, None, kind, 1.0, n)[0]
    l = R.log_gram(X, Y, kind, 1.0, n)
    assert np.isfinite(l).all() and np.isfinite(a).all() and np.isfinite(b).all(), "a pair or a diagonal of this case has K <= 0"
    assert max(a.max(), b.max(), l.max()) < 85.0, "K(x, x) of this case does not fit fp32"
    if fwd:
        return X, Y, None, np.exp(l - 0.5 * a[:, None] - 0.5 * b[None, :]), None, None
    w = None if unit else weights(len(X), len(Y), n + len(X))
    wr = np.ones((len(X), len(Y))) if unit else w
    wr = wr + wr.T if sym else wr
    if same:  # (see the head of tests/test_gpu_normalized.py)
        wr = wr - np.diag(np.diag(wr))
    Kh, gX, _ = R.normalized_gram_and_grads(X, Y, wr, kind, 1.0, n)
    t1, t2 = NF.terms(X, Y, w, kind, 1.0, n, sym, same)
    top = max(np.abs(t1).max(), np.abs(t2).max())
    assert top <= 2.0 * np.abs(gX).max(), ("the two terms cancel in this case", top, np.abs(gX).max())
    return X, Y, w, Kh, gX, G_BOUND * (np.abs(t1).max() + np.abs(t2).max())


def dev(a, io, gpu):
    return None if a is None else torch.as_tensor(a, dtype=io, device=gpu)


def launch(gpu, name, mode, io, unit=False):
    """the flagged launch of a case in a mode -> (K^, gX or None)"""
    n, kind, kw = SHAPES[name][4:7]
    X, Y, w, _, _, _ = reference(name, mode, unit)
    Xt, wt = dev(X, io, gpu), dev(w, io, gpu)
    Yt = Xt if mode in SAME else dev(Y, io, gpu)
    if mode.endswith("fwd"):
        return ops.gram_fwd(Xt, Yt, 1.0, n, kind, y_is_x=mode in SAME, normalized=True, **kw), None
    return ops.gram_fwd_bwd(Xt, Yt, 1.0, n, kind, wt, sym=mode.endswith("sym"), y_is_x=mode in SAME, normalized=True, **kw)


def check(what, K, gX, ref, io):
    """(K^, gX) against the reference's -> the worst fractions of the two bounds"""
    _, _, _, Kh, g_ref, g_bound = ref
    assert torch.isfinite(K).all(), what
    fk = float((np.abs(np64(K) - Kh) / np.abs(Kh)).max() / (K_BOUND + (3 * 2.0**-24 if io == F32 else 0.0)))
    fg = 0.0
    if g_ref is not None:
        assert gX is not None and torch.isfinite(gX).all(), what
        fg = float(np.abs(np64(gX) - g_ref).max() / g_bound)
    print(f"    {what}: K^ {fk:.2e} of its bound, gradient {fg:.2e} of its bound")
    assert fk <= 1.0 and fg <= 1.0, (what, fk, fg)
    return fk, fg


def case(gpu, monkeypatch, name, mode, io, unit=False):
    ref = reference(name, mode, unit)
    K, gX = launch(gpu, name, mode, io, unit)
    check(f"{name} {mode} {'f32' if io == F32 else 'f64'}{' unit' if unit else ''}", K, gX, ref, io)
    if mode in SAME:
        assert torch.equal(K, K.T)
        assert torch.equal(K.diagonal(), torch.ones(len(K), dtype=io, device=gpu))  # exactly 1.0
    # the same launch between guards, on exactly the queried bytes, misaligned, every byte 0xFF: the same bits
    with monkeypatch.context() as m:
        ws = GuardedWorkspace("ones", 1).install(m)
        K2, g2 = launch(gpu, name, mode, io, unit)
        ws.check()
        assert ws.count == 1 and ws.sizes[0] > 0
    assert torch.equal(K, K2) and (gX is None or torch.equal(gX, g2)), (name, mode)
    return K, gX


@pytest.mark.parametrize("io", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_every_route_and_edge_in_every_mode(gpu, monkeypatch, name, io):
    for mode in modes_of(name):
        case(gpu, monkeypatch, name, mode, io)


@pytest.mark.parametrize("io", [F32, F64], ids=["f32", "f64"])
def test_unit_weights_are_the_null_pointer(gpu, monkeypatch, io):
    """grad_out = NULL means ones (W' is materialised all the same), against the reference and against a tensor of ones"""
    for name, mode in (("fast_T40_d7", "ordered"), ("fast_T40_d7", "yx"), ("dyad_T17_n2", "yx_sym"), ("B65", "ordered")):
        K, gX = case(gpu, monkeypatch, name, mode, io, unit=True)
        n, kind, kw = SHAPES[name][4:7]
        X, Y = reference(name, mode, True)[:2]
        Xt = dev(X, io, gpu)
        Yt = Xt if mode in SAME else dev(Y, io, gpu)
        ones = torch.ones(len(X), len(Y), dtype=io, device=gpu)
        K1, g1 = ops.gram_fwd_bwd(Xt, Yt, 1.0, n, kind, ones, sym=mode.endswith("sym"), y_is_x=mode in SAME, normalized=True, **kw)
        assert torch.equal(K, K1) and torch.equal(gX, g1)


def test_forward_only_has_the_gradient_launchs_bits_of_k(gpu):
    for name, mode in (("fast_T40_d7", "ordered"), ("quad_T65", "yx"), ("band_T10_n4", "ordered")):
        K = launch(gpu, name, mode, F32)[0]
        Kf = launch(gpu, name, "yx_fwd" if mode == "yx" else "fwd", F32)[0]
        assert torch.equal(K, Kf), name


@pytest.mark.parametrize("name", ["fast_T40_d7", "quad_T65"])
def test_agrees_with_the_long_routes_flagged_launch(gpu, name):
    """`ops.gram_long_fwd_bwd2(normalized=True)` (SIGSVGD_FLAG_NORMALIZED, fp64 log-domain sweeps) on the same inputs: the two
    routes within the fused route's bounds of each other"""
    n, kind = SHAPES[name][4:6]
    for mode in ("ordered", "yx"):
        X, Y, w, _, _, g_bound = reference(name, mode)
        K, gX = launch(gpu, name, mode, F32)
        Xt, wt = dev(X, F64, gpu), dev(w, F64, gpu)
        Kl, gl, _ = ops.gram_long_fwd_bwd2(Xt, Xt if mode == "yx" else dev(Y, F64, gpu), 1.0, n, kind, wt, y_is_x=mode == "yx",
                                           want_gradY=False, normalized=True)
        assert float(((K.double() - Kl).abs() / Kl.abs()).max()) <= K_BOUND + 3 * 2.0**-24
        assert float((gX.double() - gl).abs().max()) <= g_bound


def test_two_runs_give_equal_bits(gpu):
    for name, mode in (("fast_T9", "ordered"), ("N70", "yx_sym"), ("B130", "ordered"), ("band_T10_n4", "sym")):
        a, b = launch(gpu, name, mode, F32), launch(gpu, name, mode, F32)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), name


@pytest.mark.parametrize("mode", ["yx", "ordered", "yx_fwd"])
def test_flagged_launch_is_capturable(gpu, mode):
    """no read-back, no host sync and no allocation: the diagonal pass, the weights kernel, the unflagged launch and the finish
    kernel are captured and replayed (on the cached workspace of `ops`, which the warm-up allocates before the capture)"""
    name = "fast_T40_d7"
    X, Y, w, _, _, _ = reference(name, mode)
    Xt, wt = dev(X, F32, gpu), dev(w, F32, gpu)
    Yt = Xt if mode in SAME else dev(Y, F32, gpu)

    def run():  # (the inputs are on the device already: a copy from the host cannot be captured)
        if mode.endswith("fwd"):
            return ops.gram_fwd(Xt, Yt, 1.0, 0, RBF, y_is_x=True, normalized=True), None
        return ops.gram_fwd_bwd(Xt, Yt, 1.0, 0, RBF, wt, y_is_x=mode in SAME, normalized=True)

    want = run()
    assert torch.equal(want[0], launch(gpu, name, mode, F32)[0])
    torch.cuda.synchronize()
    s = torch.cuda.Stream(gpu)
    with torch.cuda.stream(s):
        run()  # (warm-up on the capture stream)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        got = run()
    for t in got:
        if t is not None:
            t.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert all(a is b or torch.equal(a, b) for a, b in zip(got, want))


# ---- the surface -----------------------------------------------------------------------------------------------------------------
def test_sigkernel_fused_route_is_the_launch(gpu):
    import sigsvgd_amd.sigkernel as sk

    name = "fast_T40_d7"
    X, Y, w, _, _, _ = reference(name, "ordered")
    Xt, Yt, wt = dev(X, F32, gpu), dev(Y, F32, gpu), dev(w, F32, gpu)
    kernel = sk.SigKernel(sk.RBFKernel(1.0), 0, normalize=True, normalize_route="fused")
    K, gX = launch(gpu, name, "ordered", F32)
    Kk, gk = kernel.gram_and_grad(Xt, Yt, wt)
    assert torch.equal(K, Kk) and torch.equal(gX, gk)
    Xg = Xt.clone().requires_grad_(True)
    Kc = kernel.compute_Gram(Xg, Yt)
    (gc,) = torch.autograd.grad((wt * Kc).sum(), Xg)
    assert torch.equal(Kc.detach(), K) and torch.equal(gc, gX)
    Ky, gy = launch(gpu, name, "yx_sym", F32)
    w2 = dev(reference(name, "yx_sym")[2], F32, gpu)
    Kc = kernel.compute_Gram(Xg, Xg, sym=True)
    (gc,) = torch.autograd.grad((w2 * Kc).sum(), Xg)
    assert torch.equal(Kc.detach(), Ky) and torch.equal(gc, gy)
    mmd = kernel.compute_mmd(Xt, Yt)
    Kxx, Kyy = launch(gpu, name, "yx_fwd", F32)[0], ops.gram_fwd(Yt, Yt, 1.0, 0, RBF, y_is_x=True, normalized=True)
    assert torch.equal(mmd, Kxx.mean() + Kyy.mean() - 2.0 * launch(gpu, name, "fwd", F32)[0].mean())


@pytest.mark.parametrize("update", ["manual", "adam"])
def test_graphed_svgd_with_the_normalised_kernel_is_the_eager_iteration(gpu, update):
    """three steps at N = 8, T = 16, d = 3: the captured step equals the eager iteration bit for bit"""
    from sigsvgd_amd.graph import GraphedSigSVGD

    X0 = dev(R.walks(31, 8, 16, 3, 0.3, np.float32), F32, gpu)
    s0 = dev(np.random.default_rng(5).standard_normal((8, 16, 3)), F32, gpu)
    lr = 1e-2
    g = GraphedSigSVGD(X0, inv_h=1.0, dyadic_order=0, lr=lr, update=update, normalize=True)
    g.score.copy_(s0)
    Xe = X0.clone()
    adam = ops.AdamState(Xe) if update == "adam" else None
    for it in range(3):
        g.step()
        K, gk = ops.gram_fwd_bwd(Xe, Xe, 1.0, 0, y_is_x=True, normalized=True)
        if update == "adam":
            _, Xe = ops.svgd_adam(K, s0, gk, Xe, lr, adam)
        else:
            _, Xe = ops.svgd_phi(K, s0, gk, X=Xe, lr=lr)
        torch.cuda.synchronize()
        assert torch.equal(g.K, K) and torch.equal(g.grad_k, gk), (update, it)
        assert torch.equal(g.X, Xe), (update, it)
        assert torch.equal(K.diagonal(), torch.ones(8, device=gpu))
    # and it is not the unnormalised iteration
    assert not torch.equal(g.K, ops.gram_fwd_bwd(Xe, Xe, 1.0, 0, y_is_x=True)[0])


def test_one_svgd_step_with_the_normalised_kernel_on_the_fused_route(gpu):
    """N = 6 trajectories of 20 points, d = 3, through `kernels.SignatureKernel(normalize=True, normalize_route="fused")`: the
    velocity -((K^ score - grad_k) / N) against the reference's K^ and first-slot gradient.  Bound per entry: K^'s relative
    bound through the product with the score, the gradient's bound, and the fp32 rounding of the velocity launch's sums
    ((N + 2) 2^-24 of the absolute terms), all over N."""
    import sigsvgd_amd.sigkernel as sk
    from sigsvgd_amd.inference import SVGD
    from sigsvgd_amd.kernels import SignatureKernel

    N, T, d, lr = 6, 20, 3, 1e-2
    X = R.walks(21, N, T, d, 0.3, np.float32).astype(np.float64)
    Kh, g, _ = R.normalized_gram_and_grads(X, X.copy(), np.ones((N, N)) - np.eye(N))
    assert np.isfinite(Kh).all() and (Kh > 0).all() and np.isfinite(g).all(), "a pair of this batch has K <= 0"
    t1, t2 = NF.terms(X, X.copy(), None, R.RBF, 1.0, 0, False, True)
    score = np.random.default_rng(4).standard_normal(X.shape).astype(np.float32).astype(np.float64)
    S, G = score.reshape(N, -1), g.reshape(N, -1)
    v_ref = -((Kh @ S - G) / N).reshape(X.shape)
    g_bound = G_BOUND * (np.abs(t1).max() + np.abs(t2).max())
    kernel = SignatureKernel(depth=0, static_kernel=sk.RBFKernel(1.0), normalize=True, normalize_route="fused")
    for io in (F32, F64):
        eps = 2.0**-24 if io == F32 else 0.0
        bound = (((K_BOUND + 3 * eps) * (Kh @ np.abs(S)) + g_bound + (N + 2) * eps * (Kh @ np.abs(S) + np.abs(G))) / N)
        X1, info = SVGD(kernel, optimizer_class=None, lr=lr, iter_dict_device=None).step(dev(X, io, gpu),
                                                                                      grad_log_p=dev(score, io, gpu))
        assert torch.isfinite(X1).all() and torch.isfinite(info["grad"]).all()
        assert torch.equal(info["k_xx"].diagonal(), torch.ones(N, dtype=io, device=gpu))
        frac = float((np.abs(np64(info["grad"]) - v_ref).reshape(N, -1) / bound).max())
        print(f"    velocity ({io}): {frac:.2e} of its bound")
        assert frac <= 1.0
        assert float(np.abs(np64(X1) - (X - lr * v_ref)).max()) <= lr * bound.max() + 4 * eps * np.abs(X).max()
