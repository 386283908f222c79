"""SIGSVGD_FLAG_NORMALIZED on the device: the normalised kernel K^ and the gradient of sum(w K^) from
one launch of the long route, `ops.gram_long_fwd_bwd2(..., normalized=True)`, against the fp64 restatement
`log_k_reference.normalized_gram_and_grads`, and the surface built on it: `SigKernel(normalize=True).gram_and_grad`,
`kernels.SignatureKernel(normalize=True)` and an `SVGD` step.

Every case first asserts on the reference that every pair's K and every diagonal K is > 0 (all three logarithms finite), so no
case hides behind a NaN; the seeds were chosen on the CPU for that.  The checks:

    K^        per entry within the sum of the bounds tests/test_gpu_log_k.py holds the three logarithms to against the
              reference, 1e-12 max(1, |ln K|) each (times the pair's cancellation for l, halved for a_i / 2 and b_j / 2),
              relative to K^ (an absolute error of the exponent is a relative error of exp).  With fp32 I/O one rounding to
              fp32 on top: 3 * 2^-24 relative, and where K^ is below fp32's normal range (T = 400: 8e-47 off the diagonal,
              below the smallest fp32 subnormal, stored as 0) what that rounding is there, one subnormal step 2^-149 absolute.
    gradient  within BOUND = 1e-5 of the largest entry, the long route's bound.  With Y_IS_X the yardstick is the reference with
              the diagonal weights set to zero: analytically the same (a diagonal pair's K^ is the constant 1;
              tests/test_normalized_cpu.py holds the two equal to 1e-12), but the reference forms the diagonal pair's two
              terms and lets them cancel, which leaves 1e-16 of |grad ln K(x, x)| -- far above the whole gradient where the
              off-diagonal K^ are 1e-47 (T = 400) -- while the launch leaves the pair out of both terms.  On the small shapes,
              where that residue is far below the gradient, the launch is held to the unmodified reference as well.

Every flagged launch fails on a library without the feature, which answers SIGSVGD_E_BADARG for bit 2048."""
import functools

import numpy as np
import pytest
import torch

import log_k_reference as R
from parity import np64, rel_max, signed_weights
from sigsvgd_amd import _lib, ops

pytestmark = pytest.mark.gpu

BOUND = 1e-5
F64, F32 = torch.float64, torch.float32
RBF, LINEAR = _lib.STATIC_RBF, _lib.STATIC_LINEAR
KINDS = (_lib.STATIC_RBF, _lib.STATIC_LINEAR, _lib.STATIC_IMQ, _lib.STATIC_RQ, _lib.STATIC_MATERN32, _lib.STATIC_MATERN52)

# name -> (A, B, TX, TY, d, n, step): one column of increments, a 64- and a 129-row band edge, d = 17 (past the 16 channels
# kept in registers), dyadic order 2, tiles of several pairs with ragged last tiles; T131: steps of 2.0, the running exponent
# changes in most blocks; T400: K(x, x) is about 1e44, past fp32
SHAPES = {
    "P63_Q1_d1": (2, 3, 64, 2, 1, 0, 0.5),
    "P64_Q7": (3, 2, 65, 8, 3, 0, 0.5),
    "P129_Q8": (2, 2, 130, 9, 3, 0, 0.5),
    "d17": (2, 2, 20, 12, 17, 0, 0.5),
    "order2_T18": (3, 3, 18, 18, 3, 2, 0.5),
    "A5_B9": (5, 9, 20, 14, 3, 0, 0.5),
    "T131_step2": (2, 2, 131, 131, 2, 0, 2.0),
    "T400": (2, 2, 400, 400, 3, 0, 0.5),
}
SMALL = ("P63_Q1_d1", "P64_Q7", "P129_Q8", "d17", "order2_T18", "A5_B9")
# (rough walks now and then have a pair whose discrete K is negative: these cases take the next seed whose pairs, (X, Y), (X, X)
#  and (Y, Y), are all positive)  (name, kind) -> added to the seed
SEED_BUMP = {("order2_T18", _lib.STATIC_MATERN52): 1, ("T400", RBF): 1}
MODES = ("both", "row", "col", "yx", "yx_sym", "sym", "fwd", "yx_fwd")
SAME = ("yx", "yx_sym", "yx_fwd")  # one batch in both slots


def rough(seed, B, T, d, kind=RBF, step=0.5):
    """[B, T, d] fp32-valued walks (fp32 and fp64 I/O see the same inputs); the linear kernel, whose increments are not
    bounded by 1, gets steps of 0.12 so that K stays positive"""
    step = 0.12 if kind == LINEAR else step
    return R.walks(seed, B, T, d, step, np.float32).astype(np.float64)


def inputs(name, kind=RBF):
    A, B, TX, TY, d, n, step = SHAPES[name]
    seed = sum(map(ord, name)) + 17 * kind + SEED_BUMP.get((name, kind), 0)
    return rough(seed, A, TX, d, kind, step), rough(seed + 1, B, TY, d, kind, step), n


def weights(A, B, seed):
    """signed weights of order 1 with two exact zeros (one at 2 x 2, so that both off-diagonal pairs are not without weight)"""
    w = signed_weights(A, B, seed)
    w[0, B - 1] = 0.0
    if A * B > 4:
        w[A - 1, 0] = 0.0
    return w


def dev(a, io, gpu):
    return None if a is None else torch.as_tensor(a, dtype=io, device=gpu)


@functools.lru_cache(maxsize=None)
def _logs(name, kind, same):
    """(l, a, b, cancellation of l) of a case on the reference, all finite"""
    X, Y, n = inputs(name, kind)
    Y = X if same else Y
    l, c = R.log_gram(X, Y, kind, 1.0, n), R.cancellation(X, Y, kind, 1.0, n)
    a = R.log_pair_backward(X, X, None, kind, 1.0, n)[0]
    b = a if same else R.log_pair_backward(Y, Y, None, kind, 1.0, n)[0]
    assert np.isfinite(l).all() and np.isfinite(a).all() and np.isfinite(b).all(), "a pair or a diagonal of this case has K <= 0"
    return l, a, b, c


@functools.lru_cache(maxsize=None)
def reference(name, kind, mode, diagonal_weights=False):
    """-> (X, Y, n, w, K^, gX, gY) of a case in a mode: the Y_IS_X modes have X's values in both slots, and their gX is the
    first-slot gradient at fixed second slot; SYM, with or without Y_IS_X, weights w + w^T.  diagonal_weights: the Y_IS_X modes'
    reference with the launch's own weights, diagonal included (the small shapes, where its cancellation residue is far
    below the gradient: `case` holds the launch to both)"""
    X, Y, n = inputs(name, kind)
    same = mode in SAME
    _logs(name, kind, same)  # (asserts that every K is positive)
    Y = X.copy() if same else Y
    w = weights(len(X), len(Y), n + len(X))
    if name == "T400":  # (K^ is 1e-47 off the diagonal: weights of 2^120 bring the gradient, 1e-46 under unit ones, into fp32's range)
        w = w * 2.0**120
    wr = w + w.T if "sym" in mode else w
    if same and not diagonal_weights:  # (see the head of the file)
        wr = wr - np.diag(np.diag(wr))
    Kh, gX, gY = R.normalized_gram_and_grads(X, Y, wr, kind, 1.0, n)
    return X, Y, n, w, Kh, gX, gY


def khat_tolerance(name, kind, same, io):
    unit = lambda v: 1e-12 * np.maximum(1.0, np.abs(v))
    l, a, b, c = _logs(name, kind, same)
    tol = unit(l) * c + 0.5 * unit(a)[:, None] + 0.5 * unit(b)[None, :]
    return tol + (3 * 2.0**-24 if io == F32 else 0.0)


def check_khat(what, got, ref, tol):
    assert np.isfinite(np64(got)).all(), what
    floor = 2.0**-149 if got.dtype == F32 else 0.0  # (one step of fp32's subnormals, where K^ is below its normal range)
    worst = float((np.abs(np64(got) - ref) / (np.abs(ref) * tol + floor)).max())
    print(f"    {what}: {worst:.2e} of its bound")
    assert worst <= 1.0, (what, worst)


def check_grad(what, got, ref):
    assert np.isfinite(np64(got)).all(), what
    err = rel_max(np64(got), ref)
    print(f"    {what}: {err:.2e} of the largest entry")
    assert err < BOUND, (what, err)


def launch(gpu, name, io, kind, mode):
    """the flagged launch of a case in a mode -> (K^, gX, gY, the mode's keywords, Xt, Yt, wt)"""
    X, Y, n, w, _, _, _ = reference(name, kind, mode)
    Xt, wt = dev(X, io, gpu), dev(w, io, gpu)
    Yt = Xt if "yx" in mode else dev(Y, io, gpu)
    want = {"both": (True, True), "col": (False, True), "fwd": (False, False), "yx_fwd": (False, False)}.get(mode, (True, False))
    kw = dict(sym="sym" in mode, y_is_x="yx" in mode, want_gradX=want[0], want_gradY=want[1], normalized=True)
    return (*ops.gram_long_fwd_bwd2(Xt, Yt, 1.0, n, kind, wt, **kw), kw, Xt, Yt, wt)


def case(gpu, name, io, kind=RBF, mode="both"):
    """the flagged launch of a case against the reference"""
    _, _, _, _, Kh_ref, gX_ref, gY_ref = reference(name, kind, mode)
    same = mode in SAME
    Kh, gX, gY, kw, _, _, _ = launch(gpu, name, io, kind, mode)
    check_khat(f"{name} {mode}: K^ against the reference", Kh, Kh_ref, khat_tolerance(name, kind, same, io))
    assert (gX is None) == (not kw["want_gradX"]) and (gY is None) == (not kw["want_gradY"])
    if gX is not None:
        check_grad(f"{name} {mode}: gX against the reference", gX, gX_ref)
    if gY is not None:
        check_grad(f"{name} {mode}: gY against the reference", gY, gY_ref)
    if same and gX is not None and name in SMALL:  # the issue's yardstick itself: weights on the diagonal change nothing
        check_grad(f"{name} {mode}: gX against the reference with the diagonal weights", gX,
                   reference(name, kind, mode, True)[5])
    if "yx" in mode:
        assert torch.equal(Kh, Kh.T)  # the mirror store
        assert torch.equal(Kh.diagonal(), torch.ones(len(Kh), dtype=io, device=gpu))  # exactly 1.0
    return Kh, gX, gY


# ---- the shapes, both sides --------------------------------------------------------------------------------------------------------
CASES = [(name, F64) for name in SMALL] + [("P64_Q7", F32), ("A5_B9", F32), ("order2_T18", F32)]


@pytest.mark.parametrize("name,io", CASES, ids=[f"{n}-{'f64' if io == F64 else 'f32'}" for n, io in CASES])
def test_small_shapes(gpu, name, io):
    case(gpu, name, io)


# ---- the modes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("io", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("mode", MODES)
def test_modes(gpu, mode, io):
    """both / row only / column only / Y_IS_X / Y_IS_X | SYM / SYM / forward only, on order2_T18 (A = B = 3, TX = TY); the
    outputs a mode shares with the launch of both sides (or, with Y = X, of Y_IS_X) have that launch's bits"""
    Kh, gX, gY = case(gpu, "order2_T18", io, mode=mode)
    if mode in ("row", "col", "fwd"):
        full = launch(gpu, "order2_T18", io, RBF, "both")
        assert torch.equal(Kh, full[0])
        assert gX is None or torch.equal(gX, full[1])
        assert gY is None or torch.equal(gY, full[2])
    if mode == "yx_fwd":
        assert torch.equal(Kh, launch(gpu, "order2_T18", io, RBF, "yx")[0])
    if mode == "sym" and io == F64:  # (w + w^T on two batches: the row gradient of the launch of both sides with those weights)
        X, Y, n, w, _, _, _ = reference("order2_T18", RBF, "sym")
        full = ops.gram_long_fwd_bwd2(dev(X, io, gpu), dev(Y, io, gpu), 1.0, n, RBF, dev(w + w.T, io, gpu), normalized=True)
        assert torch.equal(Kh, full[0]) and torch.equal(gX, full[1])


def test_unit_weights_are_the_null_pointer(gpu):
    """grad_out = NULL means ones, in every mode with a gradient"""
    X, Y, n = inputs("order2_T18")
    Xt, Yt = dev(X, F64, gpu), dev(Y, F64, gpu)
    ones = torch.ones(3, 3, dtype=F64, device=gpu)
    for kw in (dict(), dict(y_is_x=True), dict(y_is_x=True, sym=True)):
        Yv = Xt if kw else Yt
        a = ops.gram_long_fwd_bwd2(Xt, Yv, 1.0, n, RBF, None, normalized=True, **kw)
        b = ops.gram_long_fwd_bwd2(Xt, Yv, 1.0, n, RBF, ones, normalized=True, **kw)
        assert all(p is q or torch.equal(p, q) for p, q in zip(a, b))


# ---- every kind -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_every_kind(gpu, kind):
    case(gpu, "P64_Q7", F64, kind)
    case(gpu, "order2_T18", F64, kind, "yx")


# ---- forced rescaling and past fp32 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["both", "yx"])
def test_forced_rescaling(gpu, mode):
    """(2, 2, 131, 131, 2) at steps of 2.0: ln K(x, x) is far past the drift threshold, the exponent changes in most blocks"""
    l, a, b, _ = _logs("T131_step2", RBF, mode == "yx")
    assert a.max() > 40
    case(gpu, "T131_step2", F64, mode=mode)


@pytest.mark.parametrize("io", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("mode", ["both", "yx"])
def test_past_fp32(gpu, mode, io):
    """(2, 2, 400, 400, 3) at steps of 0.5: K(x, x) is about 1e44, past fp32, and K^ is of order 1 or far below it"""
    l, a, b, _ = _logs("T400", RBF, mode == "yx")
    assert a.max() > 88.8
    case(gpu, "T400", io, mode=mode)


# ---- the diagonal, the bits, graph capture -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("io", [F64, F32], ids=["f64", "f32"])
def test_diagonal_of_a_y_is_x_launch_is_exactly_one(gpu, io):
    for (A, T, d, n, step, kind) in [(4, 300, 3, 0, 0.5, RBF), (6, 16, 3, 0, 0.5, RBF), (5, 70, 2, 1, 0.3, _lib.STATIC_MATERN32),
                                     (3, 131, 2, 0, 2.0, RBF)]:
        Xt = dev(rough(11, A, T, d, kind, step), io, gpu)
        for kw in (dict(want_gradX=False), dict(), dict(sym=True)):
            Kh = ops.gram_long_fwd_bwd2(Xt, Xt, 1.0, n, kind, None, y_is_x=True, want_gradY=False, normalized=True, **kw)[0]
            assert torch.equal(Kh.diagonal(), torch.ones(A, dtype=io, device=gpu)), (A, T, kw, Kh.diagonal())
            assert torch.equal(Kh, Kh.T)


@pytest.mark.parametrize("mode", ["both", "yx_sym"])
def test_two_runs_give_equal_bits(gpu, mode):
    a = launch(gpu, "A5_B9" if mode == "both" else "order2_T18", F64, RBF, mode)[:3]
    b = launch(gpu, "A5_B9" if mode == "both" else "order2_T18", F64, RBF, mode)[:3]
    assert all(p is q or torch.equal(p, q) for p, q in zip(a, b))


def test_flagged_launch_is_capturable(gpu):
    """no read-back, no host sync and no allocation: the whole pipeline -- diagonal passes, the two-sided launch, the sums and the
    reductions -- is captured and replayed (on the cached workspace of `ops`, which the warm-up allocates before the capture)"""
    X, Y, n = inputs("order2_T18")
    Xt, Yt, wt = dev(X, F64, gpu), dev(Y, F64, gpu), dev(weights(3, 3, 5), F64, gpu)
    want = ops.gram_long_fwd_bwd2(Xt, Yt, 1.0, n, RBF, wt, normalized=True)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(gpu)
    with torch.cuda.stream(s):
        ops.gram_long_fwd_bwd2(Xt, Yt, 1.0, n, RBF, wt, normalized=True)  # (warm-up on the capture stream)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        got = ops.gram_long_fwd_bwd2(Xt, Yt, 1.0, n, RBF, wt, normalized=True)
    for t in got:
        t.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(got, want))


# ---- the surface ---------------------------------------------------------------------------------------------------------------------
def test_agrees_with_the_composition_of_existing_launches(gpu):
    """K^ and the gradients against `SigKernel(normalize=True).compute_Gram` + autograd, the composition of five launches
    (DESIGN.md section 5.21): 1e-12 relative for K^, 1e-9 of the largest gradient entry, fp64"""
    import sigsvgd_amd.sigkernel as sk

    kernel = sk.SigKernel(sk.RBFKernel(1.0), 0, normalize=True)
    for name in ("A5_B9", "P129_Q8"):
        X, Y, n, w, _, _, _ = reference(name, RBF, "both")
        Xg, Yg = dev(X, F64, gpu).requires_grad_(True), dev(Y, F64, gpu).requires_grad_(True)
        wt = dev(w, F64, gpu)
        Kc = kernel.compute_Gram(Xg, Yg, grad_Y=True)
        cX, cY = torch.autograd.grad((wt * Kc).sum(), (Xg, Yg))
        Kh, gX, gY = ops.gram_long_fwd_bwd2(Xg.detach(), Yg.detach(), 1.0, n, RBF, wt, normalized=True)
        assert float(((Kh - Kc.detach()).abs() / Kc.detach().abs()).max()) < 1e-12
        assert rel_max(gX, np64(cX)) < 1e-9 and rel_max(gY, np64(cY)) < 1e-9
    # one tensor in both slots, both slots differentiated: Y_IS_X | SYM.  The composition solves the diagonal pairs' two terms
    # in two launches, and they cancel only to the fp32 rounding of the stored S; the flagged launch leaves both out.  With
    # no weight on the diagonal the two do the same arithmetic (1e-9).  With weights there the composition adds, per diagonal
    # pair, two terms of size |2 w_ii grad_1 ln K(x_i, x_i)| from two gradient launches, each held to BOUND of its largest
    # entry: the two may differ by 2 BOUND times the largest such term (test_modes holds the flagged launch to the reference).
    X, _, n, w, _, _, _ = reference("order2_T18", RBF, "yx_sym")
    k2 = sk.SigKernel(sk.RBFKernel(1.0), n, normalize=True)
    dl = R.log_pair_backward(X, X, None, RBF, 1.0, n)[1]  # grad_1 ln K(x_i, x_i)
    term = max(abs(2 * w[i, i]) * np.abs(dl[i]).max() for i in range(len(X)))
    for diagonal, bound in ((False, 1e-9), (True, None)):
        wd = w if diagonal else w - np.diag(np.diag(w))
        Xg, wt = dev(X, F64, gpu).requires_grad_(True), dev(wd, F64, gpu)
        Kc = k2.compute_Gram(Xg, Xg, sym=True)
        (cX,) = torch.autograd.grad((wt * Kc).sum(), Xg)
        Kh, gX = k2.gram_and_grad(Xg.detach(), None, wt, sym=True)
        assert float(((Kh - Kc.detach()).abs() / Kc.detach().abs()).max()) < 1e-12
        err = rel_max(gX, np64(cX))
        if bound is None:
            bound = 2 * BOUND * term / float(cX.abs().max())
        print(f"    Y_IS_X | SYM against the composition, diagonal weights {diagonal}: {err:.2e} of the largest entry "
              f"(bound {bound:.1e})")
        assert err < bound
    # and gram_and_grad with a second batch: the first-slot gradient
    X, Y, n, w, _, _, _ = reference("A5_B9", RBF, "both")
    Kh, gX = kernel.gram_and_grad(dev(X, F64, gpu), dev(Y, F64, gpu), dev(w, F64, gpu))
    full = ops.gram_long_fwd_bwd2(dev(X, F64, gpu), dev(Y, F64, gpu), 1.0, n, RBF, dev(w, F64, gpu), normalized=True)
    assert torch.equal(Kh, full[0]) and torch.equal(gX, full[1])


@functools.lru_cache(maxsize=None)
def _svgd_reference(N=6, T=300, d=3):
    X = rough(21, N, T, d)
    Kh, g, _ = R.normalized_gram_and_grads(X, X.copy(), np.ones((N, N)))
    assert np.isfinite(Kh).all() and (Kh > 0).all() and np.isfinite(g).all(), "a pair of this batch has K <= 0"
    score = np.random.default_rng(4).standard_normal(X.shape).astype(np.float32).astype(np.float64)
    return X, Kh, g, score


def test_one_svgd_step_with_the_normalised_kernel(gpu):
    """N = 6 trajectories of 300 points, d = 3: K(x, x) is about 1e34 here, the unnormalised Gram matrix of no use.  One
    `SVGD.step` with `kernels.SignatureKernel(normalize=True)` gives finite updates, and its velocity is
    -((K^ score - grad_k) / N) of the reference's K^ and first-slot gradient within the gradient bound."""
    import sigsvgd_amd.sigkernel as sk
    from sigsvgd_amd.inference import SVGD
    from sigsvgd_amd.kernels import SignatureKernel

    X, Kh, g, score = _svgd_reference()
    N = len(X)
    lr = 1e-2
    v_ref = -((Kh @ score.reshape(N, -1) - g.reshape(N, -1)) / N).reshape(X.shape)
    kernel = SignatureKernel(depth=0, static_kernel=sk.RBFKernel(1.0), normalize=True)
    for io in (F32, F64):  # (fp32 particles take the fused update, fp64 ones the plain one)
        Xt = dev(X, io, gpu)
        X1, info = SVGD(kernel, optimizer_class=None, lr=lr, iter_dict_device=None).step(Xt, grad_log_p=dev(score, io, gpu))
        assert torch.isfinite(X1).all() and torch.isfinite(info["grad"]).all()
        assert torch.equal(info["k_xx"].diagonal(), torch.ones(N, dtype=io, device=gpu))
        check_grad(f"velocity ({io})", info["grad"], v_ref)
        check_grad(f"updated particles ({io})", X1, X - lr * v_ref)
